"""Shot boundaries of a video: kernel temporal segmentation (KTS) on the MI355X, and uniform segments.

Drop-in for the reference's ``segmentations`` package (``create_segments.get_segment_fn`` / ``kts_seg`` /
``uniform_seg``, ``kts.cpd_nonlin`` / ``kts.kts_segmentation``): same signatures, int64 change points, float64
scores / costs.  The scatter table and the dynamic program run in fp64 on the HIP kernels of ``csrc/vs_segment.hip``
(C ABI ``include/vs_segment.h``); the Gram of ``kts_seg`` is fp32 on the matrix pipe.  There is no CPU path: without a
HIP device every KTS call raises, as the scorer does.

Beyond the reference: ``kernel="cosine"`` / ``"rbf"`` in ``kts_seg`` / ``kts_seg_batch`` (the reference's TODO "be sure to
normalize frame features"), ``gram`` (the kernel matrices of a ragged batch in one launch, ``csrc/vs_segment_gram.hip``),
and ``cpd_auto.py``'s helpers ``eval_score`` / ``eval_cost`` / ``estimate_vmax`` / ``centering``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._call import scratch, stream_of

__all__ = ["cpd_nonlin", "kts_segmentation", "kts_seg", "kts_seg_batch", "uniform_seg", "get_segment_fn",
           "shots_from_change_points", "gram", "eval_score", "eval_cost", "estimate_vmax", "centering"]

_LMAX = 100000


def _device(x):
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.device
    if not torch.cuda.is_available():
        raise RuntimeError("KTS segmentation runs on the MI355X HIP kernels only (no CPU path for the segmentation)")
    return torch.device("cuda", torch.cuda.current_device())


def _kernel_device(x, kernel):
    """_device for a kernel of the Gram.  "cosine" and "rbf" exist on the HIP kernels only, so without a HIP device they
    are what every kernel but "dot" is in the reference: not implemented (NotImplementedError is a RuntimeError, the
    type "dot" raises there)."""
    try:
        return _device(x)
    except RuntimeError as e:
        if kernel == "dot":
            raise
        raise NotImplementedError("kernel=%r: %s" % (kernel, e)) from None


def _on_device(x, dtype, dev):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
    return t.to(device=dev, dtype=dtype).contiguous()


def _i32(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _f64(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _check_args(n, m, lmin, lmax):
    """The reference's asserts (cpd_nonlin.py), refused with a ValueError."""
    if m < 0:
        raise ValueError("ncp=%d must be >= 0" % m)
    if not n >= (m + 1) * lmin:
        raise ValueError("needs n >= (ncp + 1) * lmin (n=%d ncp=%d lmin=%d)" % (n, m, lmin))
    if not n <= (m + 1) * lmax:
        raise ValueError("needs n <= (ncp + 1) * lmax (n=%d ncp=%d lmax=%d)" % (n, m, lmax))
    if not lmax >= lmin >= 1:
        raise ValueError("needs lmax >= lmin >= 1 (lmin=%d lmax=%d)" % (lmin, lmax))


_KINDS = {"dot": _lib.VS_KTS_GRAM_DOT, "cosine": _lib.VS_KTS_GRAM_COSINE, "rbf": _lib.VS_KTS_GRAM_RBF}


def _kernel_desc(kernel, gamma, D):
    """vs_kts_kernel of (kernel, gamma): NotImplementedError for an unknown name, ValueError for a gamma that the kernel
    does not take or that is not finite and > 0.  gamma=None with "rbf" is 1 / D."""
    if kernel not in _KINDS:
        raise NotImplementedError
    if gamma is not None and kernel != "rbf":
        raise ValueError("gamma is a parameter of kernel='rbf' only (got kernel=%r)" % (kernel,))
    g = 0.0
    if kernel == "rbf":
        g = 1.0 / D if gamma is None else float(gamma)
        if not (np.isfinite(g) and g > 0):
            raise ValueError("gamma=%r must be finite and > 0" % (gamma,))
    return _lib.KtsKernel(_KINDS[kernel], 0, g)


def _segment(x, input_kind, lengths, ncp, mode, lmin=None, lmax=None, vmax=None, desc_rate=None, kern=None):
    """One vs_kts_segment call (vs_kts_segment_k with a kernel descriptor) over a packed batch on x's device.  Returns
    (cps list, scores list) as numpy."""
    lib = _lib.load()
    B = len(lengths)
    cu = _i32(np.concatenate([[0], np.cumsum(lengths)]))
    ncp = _i32(ncp)
    lmin = _i32(lmin if lmin is not None else [1] * B)
    lmax = _i32(np.minimum(np.asarray(lmax if lmax is not None else [_LMAX] * B, dtype=np.int64), 2 ** 31 - 1))
    vm = _f64(vmax if vmax is not None else [0.0] * B)
    dr = _f64(desc_rate if desc_rate is not None else [1.0] * B)
    d = int(x.shape[-1]) if input_kind == _lib.VS_KTS_FEATURES_F32 else 0
    if kern is None:
        nbytes = lib.vs_kts_workspace_bytes(_p(cu), B, d, input_kind, _p(ncp), mode)
    else:
        nbytes = lib.vs_kts_workspace_bytes_k(_p(cu), B, d, input_kind, _p(ncp), mode, C.byref(kern))
    if nbytes == 0:
        _lib.check(_lib.VS_ERR_INVALID)
    ws = scratch(nbytes, x.device)
    cps = np.zeros(max(1, int(ncp.sum())), dtype=np.int64)
    n_cps = np.zeros(B, dtype=np.int32)
    scores = np.zeros(int(ncp.sum()) + B, dtype=np.float64)
    stream = stream_of(x.device)
    if kern is None:
        _lib.check(lib.vs_kts_segment(x.data_ptr(), input_kind, d, _p(cu), B, _p(ncp), _p(lmin), _p(lmax), _p(vm), _p(dr), mode,
                                      _p(cps), _p(n_cps), _p(scores), ws.data_ptr(), nbytes, stream))
    else:
        _lib.check(lib.vs_kts_segment_k(x.data_ptr(), input_kind, d, _p(cu), B, _p(ncp), _p(lmin), _p(lmax), _p(vm), _p(dr), mode,
                                        C.byref(kern), _p(cps), _p(n_cps), _p(scores), ws.data_ptr(), nbytes, stream))
    out_c, out_s, ci, si = [], [], 0, 0
    for b in range(B):
        m = int(ncp[b])
        out_c.append(cps[ci:ci + (int(n_cps[b]) if mode == _lib.VS_KTS_AUTO else m)].copy())
        out_s.append(scores[si:si + m + 1].copy())
        ci += m
        si += m + 1
    return out_c, out_s


def _scatters(x, input_kind, n):
    lib = _lib.load()
    cu, zero = _i32([0, n]), _i32([0])
    d = int(x.shape[-1]) if input_kind == _lib.VS_KTS_FEATURES_F32 else 0
    nbytes = lib.vs_kts_workspace_bytes(_p(cu), 1, d, input_kind, _p(zero), _lib.VS_KTS_SCORES)
    if nbytes == 0:
        _lib.check(_lib.VS_ERR_INVALID)
    ws = scratch(nbytes, x.device)
    out = torch.empty((n, n), dtype=torch.float64, device=x.device)
    _lib.check(lib.vs_kts_scatters(x.data_ptr(), input_kind, d, n, out.data_ptr(), ws.data_ptr(), nbytes, stream_of(x.device)))
    return out.cpu().numpy()


def _kernel_input(K):
    """K as a device tensor of its own precision class: float64 stays double, everything else float32."""
    dev = _device(K)
    dt = K.dtype if isinstance(K, torch.Tensor) else np.asarray(K).dtype
    double = dt in (torch.float64, np.float64)
    t = _on_device(K, torch.float64 if double else torch.float32, dev)
    if t.dim() != 2 or t.shape[0] != t.shape[1]:
        raise ValueError("Kernel matrix awaited (got shape %s)" % (tuple(t.shape),))
    return t, (_lib.VS_KTS_KERNEL_F64 if double else _lib.VS_KTS_KERNEL_F32)


def cpd_nonlin(K, ncp, lmin=1, lmax=100000, backtrack=True, verbose=True, out_scatters=None):
    """Change-point detection by dynamic programming (cpd_nonlin.py): returns (cps int64 [ncp], scores float64
    [ncp + 1]), scores[k] = the best objective with k change points, +inf where unreachable.  out_scatters, if given,
    receives the scatter table J [n, n] (float64, zeros below the diagonal) in out_scatters[0]."""
    m = int(ncp)
    t, kind = _kernel_input(K)
    n = int(t.shape[0])
    _check_args(n, m, int(lmin), int(lmax))
    if verbose:
        print("Precomputing scatters...")
    if out_scatters is not None:
        out_scatters[0] = _scatters(t, kind, n)
    if verbose:
        print("Inferring best change points...")
    mode = _lib.VS_KTS_BACKTRACK if backtrack else _lib.VS_KTS_SCORES
    cps, scores = _segment(t, kind, [n], [m], mode, [int(lmin)], [int(lmax)])
    return cps[0], scores[0]


def kts_segmentation(K, ncp, vmax, desc_rate=1, **kwargs):
    """Change points with their number chosen by a penalty (cpd_auto.py): returns (cps int64 [m_best], costs float64
    [ncp + 1]), costs = scores / n + penalty.  kwargs: lmin, lmax, verbose, out_scatters, as cpd_nonlin takes them."""
    m = int(ncp)
    lmin, lmax = int(kwargs.get("lmin", 1)), int(kwargs.get("lmax", _LMAX))
    verbose = kwargs.get("verbose", True)
    t, kind = _kernel_input(K)
    n = int(t.shape[0])
    _check_args(n, m, lmin, lmax)
    if verbose:
        print("Precomputing scatters...")
    if kwargs.get("out_scatters") is not None:
        kwargs["out_scatters"][0] = _scatters(t, kind, n)
    if verbose:
        print("Inferring best change points...")
    cps, costs = _segment(t, kind, [n], [m], _lib.VS_KTS_AUTO, [lmin], [lmax], [float(vmax)], [float(desc_rate)])
    return cps[0], costs[0]


def _features(features, dev):
    f = _on_device(features, torch.float32, dev)
    if f.dim() != 2:
        raise ValueError("features must be [n, feature_dim] (got shape %s)" % (tuple(f.shape),))
    return f


def _width(f):
    shape = f.shape if hasattr(f, "shape") else np.asarray(f).shape
    return int(shape[-1]) if len(shape) else 1


def _packed(features_list, kernel="dot"):
    """(packed x [sum n, D] on the device, lengths) of a list of [n, D] feature arrays."""
    dev = _kernel_device(features_list[0], kernel)
    fs = [_features(f, dev) for f in features_list]
    D = fs[0].shape[1]
    if any(f.shape[1] != D for f in fs):
        raise ValueError("every video needs the same feature width")
    return (torch.cat(fs, 0) if len(fs) > 1 else fs[0]), [int(f.shape[0]) for f in fs]


def gram(features_list, kernel: str = "dot", gamma=None):
    """The kernel matrices of a ragged list of videos, one Gram launch for all of them: a list of device float32 [n, n]
    tensors (one array in: one tensor out).  kernel: "dot" (K = X X^T), "cosine" (rows normalised, an all-zero frame
    gives a zero row and column) or "rbf" (exp(-gamma |x_i - x_j|^2), gamma=None: 1 / D).  K is symmetric bit for bit
    and a video's K does not depend on the videos around it."""
    single = not isinstance(features_list, (list, tuple))
    feats = [features_list] if single else list(features_list)
    if not feats:
        return []
    kern = _kernel_desc(kernel, gamma, _width(feats[0]))
    x, lengths = _packed(feats, kernel)
    lib = _lib.load()
    B = len(lengths)
    cu = _i32(np.concatenate([[0], np.cumsum(lengths)]))
    nbytes = lib.vs_kts_gram_workspace_bytes(_p(cu), B, int(x.shape[1]))
    if nbytes == 0:
        _lib.check(_lib.VS_ERR_INVALID)
    ws = scratch(nbytes, x.device)
    out = torch.empty(sum(n * n for n in lengths), dtype=torch.float32, device=x.device)
    _lib.check(lib.vs_kts_gram(x.data_ptr(), int(x.shape[1]), _p(cu), B, C.byref(kern), out.data_ptr(), ws.data_ptr(), nbytes,
                               stream_of(x.device)))
    ws.record_stream(torch.cuda.current_stream(x.device))
    Ks, at = [], 0
    for n in lengths:
        Ks.append(out[at:at + n * n].view(n, n))
        at += n * n
    return Ks[0] if single else Ks


def kts_seg(features, num_seg: int, v_max: float, kernel: str = "dot", gamma=None):
    """create_segments.kts_seg: change points (int64) of X [n, D].  kernel="dot": K = X X^T, not normalised (the
    reference's only kernel); "cosine" / "rbf": see gram.  Any other name raises NotImplementedError, as the reference
    does, and so do "cosine" / "rbf" where there is no HIP device; gamma with a kernel other than "rbf" is a ValueError."""
    if kernel not in _KINDS:
        raise NotImplementedError
    return kts_seg_batch([features], num_seg, v_max, kernel=kernel, gamma=gamma)[0]


def kts_seg_batch(features_list, num_seg, v_max, lmin=1, lmax=_LMAX, kernel: str = "dot", gamma=None):
    """kts_seg over a ragged corpus in one pass: the Grams, then the scatter tables and every dynamic-program step for all
    videos together.  num_seg / v_max: one value, or one per video.  Returns a list of int64 arrays, each equal to
    kts_seg of that video alone.  kernel="dot" runs one exact-fp32 GEMM per video; "cosine" / "rbf" run the one-launch
    ragged Gram (vs_kts_segment_k)."""
    feats = list(features_list)
    if kernel not in _KINDS:
        raise NotImplementedError
    if gamma is not None and kernel != "rbf":
        raise ValueError("gamma is a parameter of kernel='rbf' only (got kernel=%r)" % (kernel,))
    if not feats:
        return []
    kern = None if kernel == "dot" else _kernel_desc(kernel, gamma, _width(feats[0]))
    x, lengths = _packed(feats, kernel)
    B = len(lengths)
    per = lambda v: list(v) if np.ndim(v) else [v] * B
    ncp, vmax, lmin, lmax = [int(v) for v in per(num_seg)], [float(v) for v in per(v_max)], per(lmin), per(lmax)
    for n, m, lo, hi in zip(lengths, ncp, lmin, lmax):
        _check_args(n, m, int(lo), int(hi))
    cps, _ = _segment(x, _lib.VS_KTS_FEATURES_F32, lengths, ncp, _lib.VS_KTS_AUTO, lmin, lmax, vmax, kern=kern)
    return cps


def eval_score(K, cps):
    """cpd_auto.eval_score: the unnormalised empirical score (sum of the kernelised scatters of the segments) of the given
    change points, from the scatter table on the device - bit-equal to cpd_nonlin's score of its own change points."""
    t, kind = _kernel_input(K)
    n = int(t.shape[0])
    c = np.ascontiguousarray(np.asarray(list(cps), dtype=np.int64).reshape(-1))
    m = int(c.size)
    if m and (c[0] < 1 or c[-1] > n - 1 or (np.diff(c) <= 0).any()):
        raise ValueError("change points must be strictly increasing in 1 .. n - 1 = %d (got %s)" % (n - 1, c.tolist()))
    lib = _lib.load()
    cu, ncp = _i32([0, n]), _i32([m])
    nbytes = lib.vs_kts_workspace_bytes(_p(cu), 1, 0, kind, _p(ncp), _lib.VS_KTS_SCORES)
    if nbytes == 0:
        _lib.check(_lib.VS_ERR_INVALID)
    ws = scratch(nbytes, t.device)
    out = np.zeros(1, dtype=np.float64)
    cbuf = c if m else np.zeros(1, dtype=np.int64)
    _lib.check(lib.vs_kts_eval_score(t.data_ptr(), kind, 0, None, _p(cu), 1, _p(cbuf), _p(ncp), _p(out), ws.data_ptr(), nbytes,
                                     stream_of(t.device)))
    return float(out[0])


def eval_cost(K, cps, score, vmax):
    """cpd_auto.eval_cost: score / N + the penalty of len(cps) change points, host arithmetic in the reference's order."""
    N = np.shape(K)[0]
    penalty = (vmax * len(cps) / (2.0 * N)) * (np.log(float(N) / len(cps)) + 1)
    return score / float(N) + penalty


def centering(K):
    """cpd_auto.centering: K - row means - column means + the mean of the row means (K symmetric)."""
    if isinstance(K, torch.Tensor):
        mean_rows = K.mean(1, keepdim=True)
        return K - mean_rows - mean_rows.T + mean_rows.mean()
    K = np.asarray(K)
    mean_rows = np.mean(K, 1)[:, np.newaxis]
    return K - mean_rows - mean_rows.T + np.mean(mean_rows)


def estimate_vmax(K_stable):
    """cpd_auto.estimate_vmax: trace(centering(K) / n) of a stable segment's kernel = the scatter of the whole segment
    over n, which is eval_score with no change point."""
    return eval_score(K_stable, []) / np.shape(K_stable)[0]


def uniform_seg(n_frames: int, sec_per_seg: int = 2, fps: int = 2):
    """create_segments.uniform_seg: segment starts every fps * sec_per_seg frames."""
    return np.arange(start=0, stop=n_frames, step=fps * sec_per_seg)


def get_segment_fn(mode: str = "uniform"):
    """create_segments.get_segment_fn: "uniform" -> uniform_seg, "kts" -> kts_seg."""
    if mode == "uniform":
        return uniform_seg
    if mode == "kts":
        return kts_seg
    raise NotImplementedError


def shots_from_change_points(cps, n_frames: int, picks):
    """Change points in sub-sampled positions -> shots [n_shots, 2] int32 of inclusive frame ranges [start, end], the
    change_points format of generate_summary / vs_eval_corpus: shot i starts at picks[cps[i - 1]] (0 for the first)
    and ends one frame before the next start (n_frames - 1 for the last).  Boundaries at frame 0 or repeated collapse."""
    picks = np.asarray(picks, dtype=np.int64)
    starts = picks[np.asarray(cps, dtype=np.int64)] if len(cps) else np.zeros(0, dtype=np.int64)
    starts = np.unique(np.concatenate([[0], starts[(starts > 0) & (starts < n_frames)]]))
    ends = np.concatenate([starts[1:] - 1, [n_frames - 1]])
    return np.stack([starts, ends], axis=1).astype(np.int32)
