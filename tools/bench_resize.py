#!/usr/bin/env python3
"""The frame resize on the device (features.resize_frames_device, include/features/vs_resize.h) against the host path it
replaces (features.resize_frames: PIL, one frame at a time, one host thread), in one process.

    python tools/bench_resize.py [--reps 30] [--out profiles/resize_bench.txt] [--once]

Two videos, both resized to size=224 (224 x 398): 320 frames of 360 x 640 and 64 frames of 1080 x 1920, random bytes.
Timed, after warm-up of every shape, as medians over --reps with min and max; where two paths are compared they ALTERNATE inside
every repeat (other work shares the host); a timing is a host clock around calls that end in a device synchronise:
  the kernel alone, frames already on the device, and its time as a multiple of its byte floor: (input + output bytes) / 6.29 TB/s,
    the copy rate the README uses
  the host resize alone (PIL on this machine's CPU), per frame
  the uploads alone: the raw frames (what the device path sends) and the resized frames (what the host path sends)
  end to end, numpy video in and numpy features out, upload included on both sides:
    get_google_net_features(resize="host") against get_google_net_features(resize="device"), seeded weights
Before anything is timed the two paths' resized frames and features are compared bit for bit at the sizes timed.
--once: one device resize of each video and nothing else (for a kernel trace or a counter run)."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

pkg = importlib.import_module("video-summarization_amd")
features = pkg.features
COPY_TBS = 6.29
VIDEOS = ((320, 360, 640), (64, 1080, 1920))
SIZE = 224


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_bench.txt"))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resize needs a HIP device: there is nothing to time without one"
    dev = torch.device("cuda:0")
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    model = None
    for n, h, w in VIDEOS:
        video = np.random.default_rng(n).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
        oh, ow = features.resize_output_size(h, w, SIZE)
        raw = torch.from_numpy(video).to(dev)
        if args.once:
            features.resize_frames_device(raw, SIZE)
            torch.cuda.synchronize(dev)
            continue
        if model is None:
            model = features.GoogLeNetFeatures()
            model.load_state_dict(features.make_state_dict(1), strict=True)
            model = model.to(dev)
        shape = dict(n=n, h=h, w=w, oh=oh, ow=ow)
        path, tile = features.resize_plan_path(dev, h, w, oh, ow)
        # the same bytes, then the same features, before any timing
        small_host = features.resize_frames(video, SIZE)
        small_dev = features.resize_frames_device(raw, SIZE)
        differ = int((small_dev.cpu().numpy() != small_host).sum())
        f_host = pkg.get_google_net_features(video, SIZE, model=model, resize="host")
        f_dev = pkg.get_google_net_features(video, SIZE, model=model, resize="device")
        emit(what="device resize against PIL on this host: bytes that differ; features (float32 words) that differ", **shape,
             bytes=differ, words=int((f_host.view(np.int32) != f_dev.view(np.int32)).sum()), path=path, tile=list(tile))
        assert differ == 0
        in_bytes, out_bytes = video.size, small_host.size
        floor_ms = (in_bytes + out_bytes) / (COPY_TBS * 1e12) * 1e3
        calls = 20
        for _ in range(3):
            features.resize_frames_device(raw, SIZE)
        (k,) = alternate([lambda: features.resize_frames_device(raw, SIZE)], args.reps, dev, calls)
        emit(what="the kernel alone (resize_frames_device, frames on the device)", **shape, calls_per_timing=calls,
             in_mb=round(in_bytes / 1e6, 1), out_mb=round(out_bytes / 1e6, 1), byte_floor_ms=round(floor_ms, 4),
             times_the_byte_floor=round(k["median_ms"] / floor_ms, 2), us_per_frame=round(k["median_ms"] * 1e3 / n, 3),
             achieved_tb_per_s=round((in_bytes + out_bytes) / (k["median_ms"] * 1e-3) / 1e12, 3), **k)
        (hst,) = alternate([lambda: features.resize_frames(video, SIZE)], max(3, args.reps // 6), dev)
        emit(what="the host resize alone (resize_frames: PIL, one thread)", **shape, ms_per_frame=round(hst["median_ms"] / n, 4),
             repeats=max(3, args.reps // 6), **hst)
        small_np = np.ascontiguousarray(small_host)
        up_raw, up_small = alternate([lambda: torch.from_numpy(video).to(dev), lambda: torch.from_numpy(small_np).to(dev)], args.reps, dev)
        emit(what="upload alone: the raw frames (device path)", **shape, mb=round(in_bytes / 1e6, 1), **up_raw)
        emit(what="upload alone: the resized frames (host path)", **shape, mb=round(out_bytes / 1e6, 1), **up_small)
        e_host, e_dev = alternate([lambda: pkg.get_google_net_features(video, SIZE, model=model, resize="host"),
                                   lambda: pkg.get_google_net_features(video, SIZE, model=model, resize="device")], args.reps, dev)
        emit(what="end to end, numpy video -> numpy features, resize=\"host\"", **shape, **e_host)
        emit(what="end to end, numpy video -> numpy features, resize=\"device\"", **shape, **e_dev)
        emit(what="end to end: device / host (median time; below 1 = the device path is faster)", **shape,
             ratio=round(e_dev["median_ms"] / e_host["median_ms"], 4))
        del raw, small_dev
    if not args.once:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
