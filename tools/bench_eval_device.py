#!/usr/bin/env python3
"""The validation step with the keyshot evaluation on the host (the default) and on the device (evaluation.EvalSet), in
one process on the 75-video corpus of tools/eval_corpus.py (30 629 sub-sampled frames, 459 435 frames, 1 500 (video, user)
pairs).

    python tools/bench_eval_device.py [--reps 30] [--out profiles/eval_device_bench.txt]

Timed, after warm-up of both paths, as medians over --reps with the two paths ALTERNATING (other work shares the host):
  val_step_batched        host clock around the call, device synchronised before and after
  the evaluation alone    host path: evaluation.eval_videos on scores that already lie in host memory (no copy counted);
                          device path: EvalSet.evaluate on scores that lie in device memory (it synchronises itself)
  EvalSet(...)            the one-off creation: the static part on the host plus its upload
The three numbers of the two paths are compared before anything is timed: they must be equal bit for bit.
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

pkg = importlib.import_module("video-summarization_amd")
harness = importlib.import_module("video-summarization_amd.harness")
evaluation = importlib.import_module("video-summarization_amd.evaluation")
corpus_mod = importlib.import_module("video-summarization_amd.corpus")
from tools.eval_corpus import corpus  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_device_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    dev = torch.device("cuda", 0)
    m = pkg.SimNet(num_heads=4, d_model=256, num_layers=4, sparsity=0.0, dropout=0.3)
    m.load_state_dict(pkg.synth.make_state_dict(256, 4, 1234))
    m = m.to(dev).eval()
    feats, targets, users = corpus()
    feats = [f.to(dev) for f in feats]
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    created = []
    for _ in range(3):
        t = time.perf_counter()
        es = evaluation.EvalSet(users, "avg", dev)
        torch.cuda.synchronize(dev)
        created.append((time.perf_counter() - t) * 1e3)
    emit(what="EvalSet creation (one-off per split)", median_ms=round(float(np.median(created)), 2), runs_ms=[round(c, 2) for c in created])

    # same results first (and the warm-up of both paths)
    host = harness.val_step_batched(m, feats, targets, users, dev)
    device = harness.val_step_batched(m, feats, targets, users, dev, eval_set=es)
    assert host[1:] == device[1:], (host, device)
    assert abs(host[0] - device[0]) < 2e-6
    with torch.no_grad():
        order, flat = corpus_mod.score_corpus(lambda x, msk: m.score(x, msk), feats, device=dev, keep_on_device=True,
                                              packed_fn=lambda x, lens: m.score_packed(x, lens))
    host_scores = {}
    at = 0
    flat_host = flat.cpu().numpy()
    for i in order:
        host_scores[i] = flat_host[at: at + int(feats[i].shape[0])].copy()
        at += int(feats[i].shape[0])
    user_dict = {i: users[i] for i in order}
    fh = evaluation.eval_videos(host_scores, user_dict, "avg")
    fd = es.evaluate(flat, videos=order)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(fh, fd))
    emit(what="results", videos=len(users), picks=int(flat.numel()), frames=int(sum(u.n_frames for u in users)),
         loss_host=host[0], loss_device=device[0], f_score=host[1], kendall=host[2], spearman=host[3], metrics_bit_equal=True)
    for _ in range(3):
        harness.val_step_batched(m, feats, targets, users, dev)
        harness.val_step_batched(m, feats, targets, users, dev, eval_set=es)

    a, b = alternate([lambda: harness.val_step_batched(m, feats, targets, users, dev),
                      lambda: harness.val_step_batched(m, feats, targets, users, dev, eval_set=es)], args.reps, dev)
    emit(what="val_step_batched, evaluation on the host (default)", **a)
    emit(what="val_step_batched, eval_set= (evaluation on the device)", **b)
    a, b, c = alternate([lambda: evaluation.eval_videos(host_scores, user_dict, "avg"),
                         lambda: evaluation.eval_videos(host_scores, user_dict, "avg", max_threads=16),
                         lambda: es.evaluate(flat, videos=order)], args.reps, dev)
    emit(what="evaluation alone, host: eval_videos (pool sized by the library)", **a)
    emit(what="evaluation alone, host: eval_videos (16 threads)", **b)
    emit(what="evaluation alone, device: EvalSet.evaluate", **c)
    with torch.no_grad():
        (s,) = alternate([lambda: corpus_mod.score_corpus(lambda x, msk: m.score(x, msk), feats, device=dev, keep_on_device=True,
                                                          packed_fn=lambda x, lens: m.score_packed(x, lens))], args.reps, dev)
    emit(what="scoring alone (scores stay on the device)", **s)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
