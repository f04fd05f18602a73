#!/usr/bin/env python3
"""R3D-18 video-level features on the device: video_features.R3D18Features.extract against the float32 restatement of the same
network (tests/r3d_ref.py) run by torch's own ops on the same GPU, in one process.  Seeded weights, uint8 frames on the device.

    python tools/bench_video_features.py [--reps 30] [--out profiles/video_features_bench.txt] [--no-torch] [--once]

Timed, after warm-up of every shape, as medians over --reps with min and max, the two paths ALTERNATING inside every repeat (other
work shares the host); a timing is a host clock around calls that end in a device synchronise:
  1 x 16 x 112 x 112 (the network's canonical clip), 1 x 320 x 122 x 217 (a 360p video at size 122) and 1 x 320 x 122 x 122
  achieved TFLOP/s (2 * multiply-adds of the 20 convs, from the plan's records: vs_r3d_flops) against the 157.3 TFLOP/s fp32-MFMA
  roof, and the plan's workspace for each shape
  the costliest convs of the 320 x 122 x 217 forward, each timed alone through vs_cnn3d_conv (device events)
  frames -> both features for one 320-frame 360p video held on the host: the upload, GoogLeNetFeatures.extract(size=224) and
  R3D18Features.extract(size=122) on the same device tensor
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

import r3d_ref as ref  # noqa: E402

pkg = importlib.import_module("video-summarization_amd")
vf, L = pkg.video_features, pkg._lib
ROOF_TFLOPS = 157.3
SHAPES = ((16, 112, 112), (320, 122, 217), (320, 122, 122))


def clock(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3


def alternate(fns, reps, dev):
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ts[k].append(clock(fn, dev))
    return [dict(median_ms=round(float(np.median(t)), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4)) for t in ts]


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def conv_layers(t, h, w):
    """[(prefix, cin, cout, (kt, ks), (st, ss), (pt, ps), (t, h, w) in, (t, h, w) out)] of the 20 convs in execution order"""
    rows, cur = [], (t, h, w)
    block_in = None
    for prefix, cout, cin, (kt, ks), (st, ss), (pt, ps) in vf.conv_table():
        if prefix.endswith("conv1"):
            block_in = cur
        src = block_in if prefix.endswith("downsample") else cur
        dst = (out_size(src[0], kt, st, pt), out_size(src[1], ks, ss, ps), out_size(src[2], ks, ss, ps))
        rows.append((prefix, cin, cout, (kt, ks), (st, ss), (pt, ps), src, dst))
        if not prefix.endswith("downsample"):
            cur = dst
    return rows


def layer_flops(row):
    _, cin, cout, (kt, ks), _, _, _, (to, ho, wo) = row
    return 2 * to * ho * wo * cout * cin * kt * ks * ks


def time_layers(t, h, w, dev, reps):
    """each conv of the forward alone: median ms over reps, from device events"""
    lib = L.load()
    rows = []
    g = torch.Generator().manual_seed(1)
    for row in conv_layers(t, h, w):
        name, cin, cout, (kt, ks), (st, ss), (pt, ps), (ti, hi, wi), (to, ho, wo) = row
        first = name == "stem"
        x = (torch.randint(0, 256, (1, ti, hi, wi, 3), generator=g, dtype=torch.uint8) if first else torch.randn(1, ti, hi, wi, cin, generator=g)).to(dev)
        keep = [v.to(dev) for v in (torch.randn(cout, cin, kt, ks, ks, generator=g) * 0.05, torch.ones(cout), torch.zeros(cout), torch.zeros(cout),
                                     torch.ones(cout))]
        P = L.Cnn3dConvParams()
        for f, v in zip(("weight", "gamma", "beta", "running_mean", "running_var"), keep):
            setattr(P, f, v.data_ptr())
        packed = torch.empty(lib.vs_cnn3d_packed_floats(cout, cin, kt, ks), dtype=torch.float32, device=dev)
        out = torch.empty((1, to, ho, wo, cout), dtype=torch.float32, device=dev)
        res = torch.randn(out.shape, generator=g).to(dev) if name.endswith("conv2") else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(lib.vs_cnn3d_pack_conv(C.byref(P), cout, cin, kt, ks, packed.data_ptr(), stream))
        kind = L.VS_CNN3D_INPUT_U8_NDHWC if first else L.VS_CNN3D_INPUT_F32_NDHWC
        relu = 0 if name.endswith("downsample") else 1

        def run():
            L.check(lib.vs_cnn3d_conv(x.data_ptr(), kind, 1, ti, hi, wi, cin, packed.data_ptr(), cout, kt, ks, st, ss, pt, ps,
                                      None if res is None else res.data_ptr(), relu, out.data_ptr(), stream))

        run()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); run(); b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        ms = float(np.median(ts))
        flops = layer_flops(row)
        rows.append(dict(layer=name, shape="%dx%dx%d %d->%d k%dx%dx%d s%d" % (ti, hi, wi, cin, cout, kt, ks, ks, ss), median_ms=round(ms, 4),
                         tflops=round(flops / ms / 1e9, 2), share_of_roof=round(flops / ms / 1e9 / ROOF_TFLOPS, 3)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_features_bench.txt"))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    dev = torch.device("cuda", 0)
    lib = L.load()
    sd = vf.make_state_dict(21)
    model = vf.R3D18Features()
    model.load_state_dict(sd, strict=True)
    model = model.to(dev)
    g = torch.Generator().manual_seed(2)
    frames = {s: torch.randint(0, 256, (1,) + s + (3,), generator=g, dtype=torch.uint8).to(dev) for s in SHAPES}
    if args.once:
        for s in SHAPES:
            model.extract(frames[s])
            model.extract(frames[s])
        torch.cuda.synchronize(dev)
        return
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        with open(args.out, "w") as f:          # rewritten after every line: a run that is cut short keeps what it measured
            f.write("\n".join(lines) + "\n")

    sd32 = ref.cast(sd, torch.float32, dev)

    def torch_way(s):
        with torch.no_grad():
            return ref.forward(sd32, ref.normalise(frames[s], torch.float32))

    emit(what="setting", weights="seeded (make_state_dict(21)), not a Kinetics checkpoint", gpus=1, reps=args.reps, roof_tflops=ROOF_TFLOPS)
    have_torch = not args.no_torch
    if have_torch:
        try:
            for s in SHAPES:
                t = time.perf_counter()
                want = torch_way(s)
                torch.cuda.synchronize(dev)
                emit(what="torch's first forward (its library picks its convolution algorithms here)", shape=s, seconds=round(time.perf_counter() - t, 1))
                got = model.extract(frames[s])
                d = ((got - want).abs().max() / want.abs().max()).item()
                emit(what="ours against torch's float32 forward on this GPU, distance / max |torch|", shape=s, distance=d)
                assert d < 1e-4, d
                del want
        except Exception as e:       # the library behind torch's convolution is absent or cannot run here
            have_torch = False
            emit(what="torch's convolution cannot run on this machine: ours is reported alone", error=repr(e)[:300])
    for s in SHAPES:
        flops = lib.vs_r3d_flops(1, *s)
        assert flops == sum(layer_flops(r) for r in conv_layers(*s))
        emit(what="work and workspace, from the plan", shape=s, tflop=round(flops / 1e12, 4), workspace_mb=round(lib.vs_r3d_workspace_bytes(1, *s) / 1e6, 1))
        fns = [lambda: model.extract(frames[s])] + ([lambda: torch_way(s)] if have_torch else [])
        for fn in fns:
            for _ in range(3):
                fn()
        res = alternate(fns, args.reps, dev)
        for who, r in zip(("ours: R3D18Features.extract", "torch: float32 restatement, torch ops"), res):
            tf = flops / r["median_ms"] / 1e9
            emit(what=who, shape=s, tflops=round(tf, 2), share_of_fp32_mfma_roof=round(tf / ROOF_TFLOPS, 4), **r)
        if have_torch:
            emit(what="ours / torch (median time; below 1 = ours is faster)", shape=s, ratio=round(res[0]["median_ms"] / res[1]["median_ms"], 3))
    big = SHAPES[1]
    rows = sorted(time_layers(*big, dev, 10), key=lambda r: -r["median_ms"])
    total = sum(r["median_ms"] for r in rows)
    emit(what="the 20 convs of the 320 x 122 x 217 forward, each timed alone: sum", ms=round(total, 3))
    for r in rows[:8]:
        emit(what="costliest convs", share_of_conv_time=round(r["median_ms"] / total, 3), **r)

    # frames -> both features for one 320-frame 360p video, the upload included
    video = torch.randint(0, 256, (320, 360, 640, 3), generator=g, dtype=torch.uint8)
    goog = pkg.GoogLeNetFeatures()
    goog.load_state_dict(pkg.features.make_state_dict(11), strict=True)
    goog = goog.to(dev)
    held = {}

    def upload():
        held["frames"] = video.to(dev)

    def per_frame():
        return goog.extract(held["frames"], size=224)

    def video_level():
        return model.extract(held["frames"], size=122)

    for _ in range(2):
        upload(); per_frame(); video_level()
    up, a, b = alternate([upload, per_frame, video_level], max(5, args.reps // 3), dev)
    emit(what="360p video, 320 frames: upload of the uint8 frames (%.0f MB, pageable host memory)" % (video.numel() / 1e6), **up)
    emit(what="360p video: GoogLeNetFeatures.extract(size=224) -> [320, 1024]", **a)
    emit(what="360p video: R3D18Features.extract(size=122) -> [1, 512]", **b)
    both = up["median_ms"] + a["median_ms"] + b["median_ms"]
    emit(what="360p video: frames -> both features, one upload (sum of the three medians); a second upload would add its time again",
         ms=round(both, 2), second_upload_share=round(up["median_ms"] / (both + up["median_ms"]), 4))


if __name__ == "__main__":
    main()
