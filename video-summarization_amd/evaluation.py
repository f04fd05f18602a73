"""Keyshot evaluation of the scorer's output — drop-in for the reference ``evaluation`` package.

Same call surface as reference ``src/evaluation/compute_metrics.py:42`` ``eval_metrics(data, user_dict)``
(called from ``train.py:150``): ``data`` maps video name -> per-(sub-sampled)-frame scores, ``user_dict``
maps video name -> a record with ``user_summary, user_scores, change_points, n_frames, picks``
(reference ``data/dataset.py:146-154``).  The work (up-sampling, float32 shot means, 0/1 knapsack,
F-score, Kendall tau / Spearman rho) runs in host C++ (``csrc/vs_eval.cpp``) through the C ABI of
``include/vs_eval.h``; there is no Python fallback.  ``EvalSet`` is the same evaluation from scores that are still
on the device (``include/vs_eval_device.h``, ``csrc/vs_eval_device.hip``): opt-in, bit-equal results.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._call import on_stream, scratch


def _i32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.int32)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def upsample(scores, n_frames, positions) -> np.ndarray:
    """compute_metrics.py:19-39."""
    lib = _lib.load()
    s, pos = _f32(scores), _i32(positions)
    out = np.empty(int(n_frames), dtype=np.float32)
    _lib.check(lib.vs_eval_upsample(_p(s), s.size, _p(pos), pos.size, int(n_frames), _p(out)))
    return out


def knapSack(W, wt, val, n):
    """knapsack_implementation.py:1-30 -> list of selected shot indices."""
    lib = _lib.load()
    w = _i32(wt)[:n]
    v = np.ascontiguousarray(np.asarray(val, dtype=np.float64)[:n])
    sel = np.empty(max(n, 1), dtype=np.int32)
    cnt = C.c_int32()
    _lib.check(lib.vs_eval_knapsack(int(W), _p(w), _p(v), int(n), _p(sel), C.byref(cnt)))
    return sel[: cnt.value].tolist()


def generate_summary(all_shot_bound, all_scores, all_nframes, all_positions):
    """generate_summary.py:6-57 -> list of int8 summaries, one per video."""
    lib = _lib.load()
    out = []
    for sb, sc, nf, pos in zip(all_shot_bound, all_scores, all_nframes, all_positions):
        sb, sc, pos = _i32(sb), _f32(sc), _i32(pos)
        n = int(sb[-1, 1]) + 1
        summary = np.empty(n, dtype=np.int8)
        _lib.check(lib.vs_eval_generate_summary(_p(sc), sc.size, _p(pos), pos.size, int(nf), _p(sb), sb.shape[0],
                                                _p(summary), n))
        out.append(summary)
    return out


def evaluate_summary(predicted_summary, user_summary, eval_method):
    """evaluation_metrics.py:4-33."""
    lib = _lib.load()
    s = np.ascontiguousarray(np.asarray(predicted_summary), dtype=np.int8)
    us = np.ascontiguousarray(np.asarray(user_summary), dtype=np.int8)
    f = C.c_double()
    _lib.check(lib.vs_eval_fscore(_p(s), s.size, _p(us), us.shape[0], us.shape[1], 1 if eval_method == "max" else 0,
                                  C.byref(f)))
    return f.value


def evaluate_scores(predicted_scores, user_scores):
    """compute_correlation.py:4-15 -> (mean Kendall tau, mean Spearman rho)."""
    lib = _lib.load()
    ps = _f32(predicted_scores)
    us = np.ascontiguousarray(np.asarray(user_scores), dtype=np.float64)
    if us.shape[1] != ps.size:
        raise ValueError("user_scores has %d frames, prediction %d" % (us.shape[1], ps.size))
    k, s = C.c_double(), C.c_double()
    _lib.check(lib.vs_eval_rank_correlation(_p(ps), ps.size, _p(us), us.shape[0], C.byref(k), C.byref(s)))
    return k.value, s.value


def _video_record(r, keep, scores, u, eval_method, name):
    """Fills one vs_eval_video from a reference user record (`scores` None: a record for EvalSet)."""
    pos, cp = _i32(u.picks).reshape(-1), _i32(u.change_points)
    us = np.ascontiguousarray(np.asarray(u.user_summary), dtype=np.int8)
    uf = np.asarray(u.user_scores)
    uf = np.ascontiguousarray(uf, dtype=np.float32 if uf.dtype == np.float32 else np.float64)
    if uf.ndim != 2 or uf.shape[1] != int(u.n_frames):
        raise ValueError("user_scores of %r has shape %r, n_frames %d" % (name, uf.shape, int(u.n_frames)))
    if us.ndim != 2 or cp.ndim != 2 or cp.shape[1] != 2:
        raise ValueError("user_summary / change_points of %r have shapes %r / %r" % (name, us.shape, cp.shape))
    keep.append((scores, pos, cp, us, uf))
    r.scores = _p(scores) if scores is not None else None
    r.positions, r.change_points, r.user_summary, r.user_scores = _p(pos), _p(cp), _p(us), _p(uf)
    r.n_scores, r.n_positions, r.n_frames, r.n_shots = (scores.size if scores is not None else pos.size), pos.size, int(u.n_frames), cp.shape[0]
    r.n_users, r.user_len, r.n_score_users, r.use_max = us.shape[0], us.shape[1], uf.shape[0], 1 if eval_method == "max" else 0
    r.user_scores_f32 = 1 if uf.dtype == np.float32 else 0


def eval_videos(data, user_dict, eval_method="avg", max_threads=0):
    """The per-video results of eval_metrics: (f_score, kendall, spearman) arrays in the key order of `data`.
    ONE C call (vs_eval_corpus): every video and every (video, user) rank correlation runs on one bounded pool of host
    threads inside the library - no Python per video in the timed part, no nested pools."""
    lib = _lib.load()
    keys = list(data.keys())
    n = len(keys)
    recs = (_lib.EvalVideo * max(n, 1))()
    keep = []                                       # the arrays the records point into
    for j, k in enumerate(keys):
        _video_record(recs[j], keep, _f32(data[k]).reshape(-1), user_dict[k], eval_method, k)
    f, kt, sp = (np.empty(n, dtype=np.float64) for _ in range(3))
    _lib.check(lib.vs_eval_corpus(recs, n, int(max_threads), _p(f), _p(kt), _p(sp)))
    return f, kt, sp


def eval_metrics(data, user_dict):
    """compute_metrics.py:42-92 -> (mean F-score ['avg' protocol, :43], mean Kendall tau, mean Spearman rho);
    the means are taken in key order (the result does not depend on the threads' scheduling)."""
    if not len(data):
        return float(np.mean(())), float(np.mean(())), float(np.mean(()))
    f, kt, sp = eval_videos(data, user_dict, "avg")
    return float(np.mean(f)), float(np.mean(kt)), float(np.mean(sp))


class EvalSet:
    """The keyshot evaluation of `eval_videos` from scores that are STILL ON THE DEVICE (include/vs_eval_device.h; opt-in).

    `users`: a sequence or a dict of the reference's user records (`user_summary, user_scores, change_points, n_frames,
    picks`).  Everything that does not depend on the scores is computed here, once, and uploaded; `evaluate` then runs
    three kernels over the listed videos and returns the per-video (f_score, kendall, spearman) float64 arrays - bit
    for bit what `eval_videos` gives for the same scores.  Scores must be finite.  `n_scores`: per video, the number of
    scores `evaluate` will bring (default: one per pick)."""

    def __init__(self, users, eval_method="avg", device=None, n_scores=None):
        import torch
        self._lib = _lib.load()
        self.keys = list(users.keys()) if isinstance(users, dict) else list(range(len(users)))
        self._index = {k: j for j, k in enumerate(self.keys)}
        n = len(self.keys)
        if n < 1:
            raise ValueError("EvalSet needs at least one video")
        if n_scores is not None and len(n_scores) != n:
            raise ValueError("n_scores has %d entries, users %d" % (len(n_scores), n))
        recs = (_lib.EvalVideo * n)()
        keep = []
        for j, k in enumerate(self.keys):
            _video_record(recs[j], keep, None, users[k], eval_method, k)
            if n_scores is not None:
                recs[j].n_scores = int(n_scores[j])
        self.n_scores = [int(recs[j].n_scores) for j in range(n)]
        self.n_shots = [int(recs[j].n_shots) for j in range(n)]
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        if self.device.index is None:
            self.device = torch.device(self.device.type, torch.cuda.current_device())
        self._handle = C.c_void_p()
        self._workspace = None
        self._need = (None, 0)
        with on_stream(self.device) as stream:
            _lib.check(self._lib.vs_eval_set_create(recs, n, C.c_void_p(stream), C.byref(self._handle)))

    def close(self):
        """Frees the set's host tables and device arrays (also done when the object is collected)."""
        if getattr(self, "_handle", None):
            self._lib.vs_eval_set_free(self._handle)
            self._handle = None

    __del__ = close

    def evaluate(self, scores, videos=None, return_selected=False):
        """scores: ONE device float32 tensor, the listed videos' scores concatenated, or a list of device tensors (one
        per listed video).  videos: keys (dict) or indices of the videos, default all in the set's order.
        -> (f_score, kendall, spearman) float64 [len(videos)]; with return_selected also the list of per-video int8
        arrays [n_shots], 1 where the knapsack took the shot."""
        import torch
        keys = self.keys if videos is None else list(videos)
        try:
            ids = np.array([self._index[k] for k in keys], dtype=np.int32)
        except KeyError as e:
            raise ValueError("video %r is not in this EvalSet" % (e.args[0],))
        if ids.size < 1:
            raise ValueError("no videos listed")
        if isinstance(scores, (list, tuple)):
            if len(scores) != ids.size:
                raise ValueError("%d score tensors for %d videos" % (len(scores), ids.size))
            for t, j in zip(scores, ids):
                if t.numel() != self.n_scores[j]:
                    raise ValueError("video %r: %d scores, the set expects %d" % (self.keys[j], t.numel(), self.n_scores[j]))
            scores = torch.cat([t.reshape(-1) for t in scores]) if len(scores) > 1 else scores[0].reshape(-1)
        if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32 or scores.device != self.device:
            raise ValueError("scores must be float32 tensors on %s" % (self.device,))
        want = sum(self.n_scores[j] for j in ids)
        if scores.numel() != want:
            raise ValueError("%d scores for videos that need %d" % (scores.numel(), want))
        scores = scores.contiguous().view(-1)
        lib = self._lib
        key = ids.tobytes()
        if self._need[0] != key:                      # an epoch loop lists the same videos every time
            need = lib.vs_eval_set_workspace_bytes(self._handle, _p(ids), ids.size)
            if need == 0:
                _lib.check(_lib.VS_ERR_INVALID)
            self._need = (key, need)
        need = self._need[1]
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = scratch(need, self.device)
        f, kt, sp = (np.empty(ids.size, dtype=np.float64) for _ in range(3))
        sel = np.empty(sum(self.n_shots[j] for j in ids), dtype=np.int8) if return_selected else None
        with on_stream(self.device) as stream:
            _lib.check(lib.vs_eval_set_run(self._handle, C.c_void_p(scores.data_ptr()), _p(ids), ids.size, _p(f), _p(kt), _p(sp),
                                           _p(sel) if sel is not None else None, C.c_void_p(self._workspace.data_ptr()),
                                           self._workspace.numel(), C.c_void_p(stream)))
        if not return_selected:
            return f, kt, sp
        cuts = np.cumsum([self.n_shots[j] for j in ids])[:-1]
        return f, kt, sp, np.split(sel, cuts)
