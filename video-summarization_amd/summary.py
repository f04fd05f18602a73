"""Keyshot summaries on the device: importance scores that never leave the GPU in, the per-frame summary and the list of
selected frames out (``include/vs_summary.h``, ``csrc/vs_summary.hip``) - for labeled and unlabeled videos alike.

``summarize_scores`` is the library call (one ``vs_summarize`` for a whole list of videos); ``summarize`` is the
end-to-end call for new videos (batched scoring, shots from KTS when none are given, then ``summarize_scores``);
``generate_summary``, ``get_summary`` and ``generate_video_summary_json`` are drop-ins for the functions of the same
names in the reference's ``src/generate_summary_image.py`` (:91, :55, :39).  The selection is the host library's
(``evaluation.generate_summary``) bit for bit.  There is no CPU path: host tensors raise.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

from . import _lib
from ._call import on_stream, scratch
from .corpus import packed_scorer, score_corpus
from . import evaluation


def _i32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.int32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Summary:
    """One video's summary.  summary: int8 device tensor [last_shot_end + 1]; frames: int32 device tensor [n_selected],
    the ascending indices where summary is 1 (both are views into one allocation per call); selected_shots: numpy int8
    [n_shots]; shot_means: numpy float64 [n_shots] (the float32 means the knapsack saw)."""
    __slots__ = ("summary", "frames", "selected_shots", "shot_means")

    def __init__(self, summary, frames, selected_shots, shot_means):
        self.summary, self.frames, self.selected_shots, self.shot_means = summary, frames, selected_shots, shot_means


def summarize_scores(scores, change_points, n_frames, picks, proportion=0.15, n_scores=None):
    """scores: ONE float32 device tensor, the videos' scores concatenated in order, or a list of device tensors (one per
    video).  change_points / n_frames / picks: per video, as in the reference's user records ([n_shots, 2] inclusive
    ends, int, positions of the scored frames).  n_scores: per video, how many scores it brings (default: the tensors'
    sizes for a list, one per pick for a concatenated tensor).  -> list of ``Summary``, one ``vs_summarize`` call."""
    import torch
    cps = [_i32(c) for c in change_points]
    pos = [_i32(p).reshape(-1) for p in picks]
    nf = _i32([int(n) for n in n_frames]).reshape(-1)
    n = len(cps)
    if n < 1:
        raise ValueError("no videos listed")
    if len(pos) != n or nf.size != n:
        raise ValueError("%d change_points, %d picks, %d n_frames" % (n, len(pos), nf.size))
    for v, c in enumerate(cps):
        if c.ndim != 2 or c.shape[1] != 2:
            raise ValueError("change_points of video %d have shape %r" % (v, c.shape))
    if isinstance(scores, (list, tuple)):
        if len(scores) != n:
            raise ValueError("%d score tensors for %d videos" % (len(scores), n))
        for t in scores:
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError("scores must be float32 tensors on a HIP device (there is no CPU path)")
        if n_scores is None:
            n_scores = [int(t.numel()) for t in scores]
        scores = torch.cat([t.reshape(-1) for t in scores]) if n > 1 else scores[0].reshape(-1)
    if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32 or not scores.is_cuda:
        raise ValueError("scores must be float32 tensors on a HIP device (there is no CPU path)")
    nsc = _i32([p.size for p in pos] if n_scores is None else [int(k) for k in n_scores]).reshape(-1)
    if nsc.size != n:
        raise ValueError("n_scores has %d entries for %d videos" % (nsc.size, n))
    if scores.numel() != int(nsc.sum()):
        raise ValueError("%d scores for videos that need %d" % (scores.numel(), int(nsc.sum())))
    scores = scores.contiguous().view(-1)
    dev = scores.device
    npos = _i32([p.size for p in pos])
    nsh = _i32([c.shape[0] for c in cps])
    pos_all = np.concatenate(pos) if n > 1 else pos[0]
    cps_all = np.ascontiguousarray(np.concatenate(cps, axis=0)) if n > 1 else cps[0]
    lib = _lib.load()
    need = lib.vs_summarize_workspace_bytes(n, _p(npos), _p(nf), _p(nsh), _p(cps_all), float(proportion))
    lens = [int(c[-1, 1]) + 1 for c in cps] if need else [0] * n
    if need == 0:                                   # an argument check failed: the call below repeats it for its message and status
        need = 256
    total = max(sum(lens), 1)
    out = torch.empty(total * 5, dtype=torch.uint8, device=dev)      # int32 frames first (aligned), then the int8 summary
    frames_all = out[: total * 4].view(torch.int32)
    summary_all = out[total * 4:].view(torch.int8)
    ws = scratch(need, dev)
    n_sel = np.zeros(n, dtype=np.int32)
    sel = np.zeros(int(nsh.sum()), dtype=np.int8)
    means = np.zeros(int(nsh.sum()), dtype=np.float64)
    with on_stream(dev) as stream:
        rc = lib.vs_summarize(n, _p(nsc), _p(npos), _p(nf), _p(nsh), _p(pos_all), _p(cps_all), float(proportion),
                              C.c_void_p(scores.data_ptr()), C.c_void_p(summary_all.data_ptr()), C.c_void_p(frames_all.data_ptr()),
                              _p(n_sel), _p(sel), _p(means), C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(stream))
    if rc == _lib.VS_ERR_INVALID:
        raise ValueError("libvsscore: %s" % lib.vs_last_error().decode("utf-8", "replace"))
    _lib.check(rc)
    res, at, sat = [], 0, 0
    for v in range(n):
        k = int(nsh[v])
        res.append(Summary(summary_all[at: at + lens[v]], frames_all[at: at + int(n_sel[v])], sel[sat: sat + k].copy(),
                           means[sat: sat + k].copy()))
        at += lens[v]
        sat += k
    return res


def _model_device(model):
    import torch
    for t in model.parameters():
        return t.device
    return torch.device("cuda")


def _score_on_device(model, feats, dev, max_frames):
    """The videos' sigmoid scores concatenated in order, on the device (one batched pass, packed when the model allows)."""
    _, flat = score_corpus(lambda x, m: model.score(x, m), feats, device=dev, max_frames=max_frames, packed_fn=packed_scorer(model),
                           keep_on_device=True)
    return flat


def summarize(model, features, n_frames=None, picks=None, change_points=None, num_seg=None, v_max=1.0, proportion=0.15,
              max_frames=65536, kernel="dot", gamma=None):
    """The summaries of new videos end to end.  features: list of [T_i, 1024]; picks (default arange(T_i)) and n_frames
    (default T_i) as in the reference's records; change_points: per video [n_shots, 2], or None: the shots then come
    from ONE kts_seg_batch(features, min(num_seg, T_i - 1), v_max, kernel=kernel, gamma=gamma) and
    shots_from_change_points.  The scores never visit the host.  -> list of ``Summary``."""
    import torch
    from . import segmentation
    model.eval()
    dev = _model_device(model)
    feats = [f.to(dev) for f in features]
    T = [int(f.shape[0]) for f in feats]
    picks = [np.arange(t) for t in T] if picks is None else list(picks)
    n_frames = list(T) if n_frames is None else [int(x) for x in n_frames]
    with torch.no_grad():
        flat = _score_on_device(model, feats, dev, max_frames)
        if change_points is None:
            if num_seg is None:
                raise ValueError("summarize needs change_points or num_seg (the number of KTS change points)")
            per = list(num_seg) if np.ndim(num_seg) else [num_seg] * len(T)
            cps = segmentation.kts_seg_batch(feats, [min(int(m), t - 1) for m, t in zip(per, T)], v_max, kernel=kernel,
                                             gamma=gamma)
            change_points = [segmentation.shots_from_change_points(c, nf, p) for c, nf, p in zip(cps, n_frames, picks)]
    return summarize_scores(flat, change_points, n_frames, picks, proportion, n_scores=T)


def generate_summary(predicted_dict, user_dict):
    """generate_summary_image.py:91-120: host scores in, the list of int8 summaries out (the host library)."""
    keys = list(predicted_dict.keys())
    users = [user_dict[k] for k in keys]
    return evaluation.generate_summary([u.change_points for u in users], [predicted_dict[k] for k in keys],
                                       [u.n_frames for u in users], [u.picks for u in users])


def get_summary(model, data_loader):
    """generate_summary_image.py:55-80 -> {"video_%d": [frame indices]} in loader order, on the device path: the loader is
    collected, scored in one batched pass and summarised by one summarize_scores call."""
    import torch
    model.eval()
    dev = _model_device(model)
    seen = {}                                        # keyed like the reference's score_dict / user_dict
    for feature, _, user in data_loader:
        seen[user.name] = (feature, user)
    if not seen:
        return {}
    feats = [f.reshape(-1, f.shape[-1]).to(dev) for f, _ in seen.values()]
    users = [u for _, u in seen.values()]
    with torch.no_grad():
        flat = _score_on_device(model, feats, dev, 65536)
    res = summarize_scores(flat, [u.change_points for u in users], [u.n_frames for u in users], [u.picks for u in users],
                           n_scores=[int(f.shape[0]) for f in feats])
    if len(res) > 1:                                 # ONE device-to-host copy: the records' frames are slices of one tensor
        host = torch.cat([r.frames for r in res]).cpu().numpy()
    else:
        host = res[0].frames.cpu().numpy()
    out, at = {}, 0
    for i, r in enumerate(res):
        k = int(r.frames.numel())
        out["video_%d" % i] = host[at: at + k].tolist()
        at += k
    return out


def generate_video_summary_json(model, data_loader):
    """generate_summary_image.py:39-51: writes get_summary's dict to summary.json (indent=8)."""
    summaries = get_summary(model, data_loader)
    with open("summary.json", "w") as file:
        json.dump(summaries, file, indent=8)
