#!/usr/bin/env python3
"""Keyshot summaries from scores that lie in device memory: the host way against summary.summarize_scores, in one process
on the 75-video corpus of tools/eval_corpus.py.

    python tools/bench_summary.py [--reps 30] [--out profiles/summary_bench.txt]

Timed, after warm-up of every path, as medians over --reps with the paths ALTERNATING (other work shares the host):
  (a) host        the scores are copied device-to-host, evaluation.generate_summary runs per video (host C++), then
                  np.flatnonzero per video - what a caller could do before summarize_scores existed
  (b) device      summary.summarize_scores on the scores still on the device (it synchronises itself); once as it
                  returns (summary and frames stay on the device) and once with a final .cpu() of the selected frames
  end to end      summary.summarize(model, features, num_seg=...) without change points (scoring, KTS, summary) against
                  the same steps from today's functions (score_corpus -> host, kts_seg_batch, shots_from_change_points,
                  generate_summary, flatnonzero); the stages are also timed on their own
The two paths' summaries and frame lists are compared before anything is timed: they must be equal.
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
evaluation = importlib.import_module("video-summarization_amd.evaluation")
summary = importlib.import_module("video-summarization_amd.summary")
segmentation = importlib.import_module("video-summarization_amd.segmentation")
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
    ap.add_argument("--num-seg", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    dev = torch.device("cuda", 0)
    m = pkg.SimNet(num_heads=4, d_model=256, num_layers=4, sparsity=0.0, dropout=0.3)
    m.load_state_dict(pkg.synth.make_state_dict(256, 4, 1234))
    m = m.to(dev).eval()
    feats, _, users = corpus()
    feats = [f.to(dev) for f in feats]
    T = [int(f.shape[0]) for f in feats]
    cps, nfs, picks = [u.change_points for u in users], [u.n_frames for u in users], [u.picks for u in users]
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def score():
        with torch.no_grad():
            return corpus_mod.score_corpus(lambda x, msk: m.score(x, msk), feats, device=dev, keep_on_device=True,
                                           packed_fn=lambda x, lens: m.score_packed(x, lens))[1]

    flat = score()
    cuts = np.cumsum(T)[:-1]

    def host_way(shots=cps, n_frames=nfs, positions=picks):
        per = np.split(flat.cpu().numpy(), cuts)                                   # the device-to-host copy of the scores
        out = evaluation.generate_summary(shots, per, n_frames, positions)        # host C++, one video per call
        return out, [np.flatnonzero(s) for s in out]

    def device_way(to_host=False):
        res = summary.summarize_scores(flat, cps, nfs, picks, n_scores=T)
        if to_host:
            return res, torch.cat([r.frames for r in res]).cpu()
        return res, None

    # same results first (and the warm-up of both paths)
    hs, hf = host_way()
    res, _ = device_way()
    for i in range(len(users)):
        assert np.array_equal(res[i].summary.cpu().numpy(), hs[i]) and np.array_equal(res[i].frames.cpu().numpy(), hf[i]), i
    emit(what="results", videos=len(users), picks=int(flat.numel()), frames=int(sum(nfs)), shots=int(sum(c.shape[0] for c in cps)),
         selected_frames=int(sum(f.size for f in hf)), summaries_equal=True)
    for _ in range(3):
        host_way(); device_way(); device_way(True)
    a, b, c = alternate([host_way, device_way, lambda: device_way(True)], args.reps, dev)
    emit(what="(a) host: scores D2H + evaluation.generate_summary per video + flatnonzero", **a)
    emit(what="(b) device: summarize_scores, summary and frames stay on the device", **b)
    emit(what="(b) device: summarize_scores + .cpu() of the selected frames", **c)

    # end to end without change points: scoring + KTS + summary
    ncp = [min(args.num_seg, t - 1) for t in T]
    ar = [np.arange(t) for t in T]

    def kts():
        return segmentation.kts_seg_batch(feats, ncp, 1.0)

    def shots_of(k):
        return [segmentation.shots_from_change_points(c, t, p) for c, t, p in zip(k, T, ar)]

    def old_end_to_end():
        nonlocal flat
        flat = score()
        return host_way(shots_of(kts()), T, ar)

    def new_end_to_end():
        return summary.summarize(m, feats, num_seg=args.num_seg, v_max=1.0)

    (os_, of), ns = old_end_to_end(), new_end_to_end()
    for i in range(len(users)):
        assert np.array_equal(ns[i].summary.cpu().numpy(), os_[i]) and np.array_equal(ns[i].frames.cpu().numpy(), of[i]), i
    for _ in range(2):
        old_end_to_end(); new_end_to_end()
    a, b = alternate([old_end_to_end, new_end_to_end], args.reps, dev)
    emit(what="end to end, today's functions: score + kts_seg_batch + shots + scores D2H + generate_summary + flatnonzero", **a)
    emit(what="end to end: summary.summarize (score + kts_seg_batch + shots + summarize_scores)", **b)
    k = kts()
    sh = shots_of(k)
    s1, s2, s3, s4, s5 = alternate([score, kts, lambda: shots_of(k), lambda: host_way(sh, T, ar),
                                    lambda: summary.summarize_scores(flat, sh, T, ar, n_scores=T)], args.reps, dev)
    emit(what="stage: scoring (scores stay on the device)", **s1)
    emit(what="stage: kts_seg_batch (change points come back to the host)", **s2)
    emit(what="stage: shots_from_change_points (numpy)", **s3)
    emit(what="stage: host summary of the KTS shots (scores D2H + generate_summary + flatnonzero)", **s4)
    emit(what="stage: summarize_scores of the KTS shots", **s5)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
