#!/usr/bin/env python3
"""Device-resident training sets against the DataLoader, in one process.

    python tools/bench_trainset.py [--reps 10] [--out profiles/trainset_bench.txt]

(a) one fine-tuning epoch, wall time (host clock around work that ends in a device synchronise), medians over --reps with
    the paths ALTERNATING inside every repeat (other work shares the host), min-max beside them:
      loader w0 / w4   harness.train_step_packed over DataLoader(list of (feature, target), shuffle=True, num_workers=0 / 4,
                       collate_fn=collate_fn_train_packed) - the loop as it stood before the resident sets; the padded
                       form is the loop of train.py:111-131 over collate_fn_train
      resident         harness.train_epoch_resident over data.TrainSet (uploaded once, outside the timed window)
    case 1: the reference's workload - 40 videos of about 320 frames, B = 4 (10 steps per epoch)
    case 2: 64 videos of 100-650 frames in ONE batch (1 step per epoch)
    model M-A (H4 / d256 / L4, dropout 0.3), the native Adam, an unmodified GradScaler, exact fp32.
(b) the gather alone, device events around --inner back-to-back calls of the C entry into preallocated outputs, per call;
    bytes moved (rows read + rows written, features + targets + mask) over that time as a fraction of the 6.29 TB/s float4
    copy rate of MI355X_MICROARCH.md; against torch.cat over the same device slices and, padded, pad_sequence on device
    tensors with the mask compare, in the same run.  Every figure is taken twice.  "same buffers": each call reads the same
    arena rows and writes the same outputs - 11 MB (B = 4) and 207-274 MB (B = 64) per call next to a 256 MB Infinity
    Cache, so BOTH batch shapes are served partly from cache and the fraction is not an HBM rate (torch.cat and
    pad_sequence profit alike).  "rotating": the calls take turns over clones of the set and of the outputs whose
    footprint is several times the cache, so every call's rows come from HBM.  The B = 4 figures are launch latency
    either way, not bandwidth.
The resident batches are compared with the loader's (bit-equal) before anything is timed.
"""
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
from torch.nn.utils.rnn import pad_sequence  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

pkg = importlib.import_module("video-summarization_amd")
data = importlib.import_module("video-summarization_amd.data")
harness = importlib.import_module("video-summarization_amd.harness")
_lib = pkg._lib
COPY_RATE = 6.29e12          # bytes/s, MI355X_MICROARCH.md: measured float4 copy


def clock(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3


def alternate(fns, reps, dev):
    """median ms, min and max of each callable, the callables taking turns inside every repeat"""
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ts[k].append(clock(fn, dev))
    return [dict(median_ms=round(float(np.median(t)), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3)) for t in ts]


def device_us(fn, inner, dev):
    """microseconds per call: device events around `inner` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1e3 / inner


def make_videos(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(t, 1024, generator=g).abs() * 0.5, torch.rand(t, generator=g)) for t in lengths]


def padded_loader_epoch(model, optim, loader, scaler, dev):
    """train.py:111-131 over collate_fn_train"""
    model.train()
    total, n = 0.0, 0
    for feature, target in loader:
        feature, target = feature.to(dev), target.to(dev)
        mask = (feature[:, :, 0] == 1000)
        with torch.amp.autocast("cuda"):
            pred, _ = model(feature, mask)
            loss = pkg.mse_with_mask_loss(pred, target, mask)
        optim.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(optim)
        scaler.update()
        total, n = total + loss.item(), n + 1
    return total / max(n, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainset_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    lines = []

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(**row):                       # the file grows with every row: a run that is cut short keeps what it measured
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    torch.manual_seed(1234)
    m = pkg.SimNet(num_heads=4, d_model=256, num_layers=4, sparsity=0.0, dropout=0.3).to(dev)
    m.load_state_dict(pkg.synth.make_state_dict(256, 4, 1234))
    opt = pkg.Adam(m.parameters(), lr=1e-5, weight_decay=0.01).attach(m)
    scaler = torch.amp.GradScaler("cuda")

    rng = np.random.Generator(np.random.PCG64(7))
    cases = [("case 1: 40 videos of ~320 frames, B = 4", [int(t) for t in rng.integers(270, 371, size=40)], 4),
             ("case 2: 64 videos of 100-650 frames, B = 64", pkg.synth.corpus_lengths(64, 7), 64)]
    for name, lengths, bs in cases:
        videos = make_videos(lengths, 11)
        ts = data.TrainSet([f for f, _ in videos], [t for _, t in videos], dev)
        emit(what=name, videos=len(lengths), frames=int(sum(lengths)), longest=max(lengths), resident_bytes=ts.nbytes,
             steps_per_epoch=-(-len(lengths) // bs))

        # the same batches first (and the warm-up of every path)
        for packed in (True, False):
            torch.manual_seed(5)
            want = list(DataLoader(videos, shuffle=True, batch_size=bs, collate_fn=data.collate_fn_train_packed if packed else data.collate_fn_train))
            torch.manual_seed(5)
            got = list(ts.epoch(bs, packed=packed))
            assert len(want) == len(got)
            for w, g in zip(want, got):
                assert torch.equal(g[0].cpu(), w[0]) and torch.equal(g[1].cpu(), w[1])
                assert (g[2] == w[2]) if packed else torch.equal(g[2].cpu(), w[0][:, :, 0] == 1000)
        emit(what="resident batches equal the loader's, packed and padded", equal=True)

        def loaders(collate):
            return [DataLoader(videos, shuffle=True, batch_size=bs, num_workers=w, collate_fn=collate) for w in (0, 4)]

        p0, p4 = loaders(data.collate_fn_train_packed)
        q0, q4 = loaders(data.collate_fn_train)
        paths = [
            ("packed, loader num_workers=0 + train_step_packed", lambda: harness.train_step_packed(m, opt, p0, scaler, dev)),
            ("packed, loader num_workers=4 + train_step_packed", lambda: harness.train_step_packed(m, opt, p4, scaler, dev)),
            ("packed, TrainSet + train_epoch_resident", lambda: harness.train_epoch_resident(m, opt, ts, scaler, bs, packed=True)),
            ("padded, loader num_workers=0 + train.py loop", lambda: padded_loader_epoch(m, opt, q0, scaler, dev)),
            ("padded, loader num_workers=4 + train.py loop", lambda: padded_loader_epoch(m, opt, q4, scaler, dev)),
            ("padded, TrainSet + train_epoch_resident", lambda: harness.train_epoch_resident(m, opt, ts, scaler, bs, packed=False)),
        ]
        for _, fn in paths:
            fn(); fn()
        for (label, _), r in zip(paths, alternate([fn for _, fn in paths], args.reps, dev)):
            emit(what="(a) epoch wall time: " + label, reps=args.reps, **r)

        # (b) the gather alone: the first batch of an unshuffled epoch
        plan = data.epoch_plan(lengths, bs, shuffle=False)
        ids, blens, start, t_max = plan.batches[0], plan.lengths[0], plan.out_start[0], plan.t_max[0]
        B, rows = len(ids), start[-1]
        ids_d = torch.tensor(ids, dtype=torch.int32, device=dev)
        start_d = torch.tensor(start, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        vs = ts.video_start_host
        bytes_packed = 2 * rows * (1024 + 1) * 4
        bytes_padded = rows * (1024 + 1) * 4 + B * t_max * ((1024 + 1) * 4 + 1)
        # clones for the rotating figures: their footprint (arena + outputs) is at least 3x the 256 MB cache
        K = int(min(64, max(4, -(-(768 << 20) // bytes_packed))))
        sets = [(ts.arena, ts.side)] + [(ts.arena.clone(), ts.side.clone()) for _ in range(K - 1)]
        outs = [(torch.empty((rows, 1024), device=dev), torch.empty((rows,), device=dev), torch.empty((B, t_max, 1024), device=dev),
                 torch.empty((B, t_max), device=dev), torch.empty((B, t_max), dtype=torch.uint8, device=dev)) for _ in range(K)]
        slices = [([a[vs[i]: vs[i + 1]] for i in ids], [s_[vs[i]: vs[i + 1]] for i in ids]) for a, s_ in sets]
        turn = [0]

        def pick(rotate):
            turn[0] = (turn[0] + 1) % K if rotate else 0
            return turn[0]

        def g_packed(rotate=False):
            k = pick(rotate)
            (a, s_), (x, y, _, _, _) = sets[k], outs[k]
            _lib.check(lib.vs_batch_gather_packed(a.data_ptr(), s_.data_ptr(), ts.video_start.data_ptr(), len(ts),
                                                  ids_d.data_ptr(), start_d.data_ptr(), B, rows, 1024, x.data_ptr(), y.data_ptr(), st))

        def g_padded(rotate=False):
            k = pick(rotate)
            (a, s_), (_, _, xp, yp, mp) = sets[k], outs[k]
            _lib.check(lib.vs_batch_gather_padded(a.data_ptr(), s_.data_ptr(), ts.video_start.data_ptr(), len(ts),
                                                  ids_d.data_ptr(), start_d.data_ptr(), B, t_max, t_max, 1000.0, 1024, xp.data_ptr(),
                                                  yp.data_ptr(), mp.data_ptr(), st))

        def t_cat(rotate=False):
            fs, tg = slices[pick(rotate)]
            return torch.cat(fs, dim=0), torch.cat(tg, dim=0)

        def t_pad(rotate=False):
            fs, tg = slices[pick(rotate)]
            f = pad_sequence(fs, batch_first=True, padding_value=1000)
            return f, pad_sequence(tg, batch_first=True, padding_value=1000), f[:, :, 0] == 1000

        g_packed(); g_padded()
        x, _, xp, _, mp = outs[0]
        assert torch.equal(x, t_cat()[0]) and torch.equal(xp, t_pad()[0]) and torch.equal(mp.view(torch.bool), t_pad()[2])
        for label, fn, nbytes in (("vs_batch_gather_packed", g_packed, bytes_packed), ("torch.cat of the slices (features, targets)", t_cat, bytes_packed),
                                  ("vs_batch_gather_padded", g_padded, bytes_padded),
                                  ("pad_sequence on device tensors (features, targets) + mask compare", t_pad, bytes_padded)):
            for rotate in (False, True):
                call = (lambda f=fn, r=rotate: f(r))
                for _ in range(K + 5):
                    call()
                us = sorted(device_us(call, args.inner, dev) for _ in range(5))
                emit(what="(b) gather alone, B = %d, %s: %s" % (B, "rotating over %d clones" % K if rotate else "same buffers", label),
                     rows=int(rows), t_max=int(t_max), bytes_moved=int(nbytes),
                     median_us=round(us[2], 2), min_us=round(us[0], 2), max_us=round(us[4], 2),
                     fraction_of_copy_rate=round(nbytes / (us[2] * 1e-6) / COPY_RATE, 3))
        del sets, outs, slices, x, xp, mp
        del ts



if __name__ == "__main__":
    main()
