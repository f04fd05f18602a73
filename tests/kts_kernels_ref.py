"""Float64 definitions of the KTS kernel matrices (include/vs_segment.h: dot, cosine, rbf), written from the maths, and the
planted-shot features of tests/golden/kts_kernels_golden.npz.  Shared by the golden generator and the tests.

g = X X^T, s_i = sum_k x_ik^2.  cosine: clip(g_ij / (|x_i| |x_j|), -1, 1), diagonal 1 (0 for an all-zero frame, whose
row and column are 0).  rbf: exp(-gamma max(0, s_i + s_j - 2 g_ij)), diagonal 1.  gram32=True takes g from a numpy
float32 matmul and applies the same double epilogue: the yardstick of what an fp32 Gram costs (err32).
"""
import numpy as np

KINDS = ("dot", "cosine", "rbf")


def kernel64(x, kind, gamma=None, gram32=False):
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    x64 = x.astype(np.float64)
    g = np.dot(x, x.T).astype(np.float64) if gram32 else x64 @ x64.T
    s = (x64 * x64).sum(1)
    if kind == "dot":
        return g
    if kind == "cosine":
        inv = np.where(s > 0, 1.0 / np.sqrt(np.where(s > 0, s, 1.0)), 0.0)
        K = np.clip(g * inv[:, None] * inv[None, :], -1.0, 1.0)
        np.fill_diagonal(K, (s > 0).astype(np.float64))
        return K
    assert kind == "rbf"
    gamma = 1.0 / x.shape[1] if gamma is None else float(gamma)
    K = np.exp(-gamma * np.maximum(s[:, None] + s[None, :] - 2.0 * g, 0.0))
    np.fill_diagonal(K, 1.0)
    return K


def planted_shots(lengths, D, noise, seed):
    """One centroid (standard normal + 1) per shot, Gaussian noise on every frame; float32 [sum(lengths), D]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cent = rng.standard_normal((len(lengths), D)) + 1.0
    lab = np.repeat(np.arange(len(lengths)), lengths)
    return (cent[lab] + noise * rng.standard_normal((len(lab), D))).astype(np.float32)


def eval_cost(n, m, score, vmax):
    """cpd_auto.eval_cost restated: score / n + the penalty of m change points."""
    return score / float(n) + (vmax * m / (2.0 * n)) * (np.log(float(n) / m) + 1)
