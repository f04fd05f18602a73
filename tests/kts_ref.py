"""Float64 restatement of kernel temporal segmentation, written from the maths (vectorised numpy, no reference code).

J[s, e] = scatter of frames s..e = sum_i K[i, i] - (sum_{i, j in [s, e]} K[i, j]) / (e - s + 1), from the diagonal
prefix K1 and the 2-D prefix K2.  I[k, l] = best objective of k change points over the first l frames:
I[0, l] = J[0, l - 1] for lmin <= l < lmax; I[k, l] = min over t in [max(k lmin, l - lmax), l - lmin] of
I[k - 1, t] + J[t, l - 1], applied only below 1e100 (else 1e100), the smallest t on ties; everything else 1e101.
"""
import numpy as np


def scatters(K):
    K = np.asarray(K, dtype=np.float64)
    n = K.shape[0]
    K1 = np.concatenate([[0.0], np.cumsum(np.diag(K))])
    K2 = np.zeros((n + 1, n + 1))
    K2[1:, 1:] = np.cumsum(np.cumsum(K, 0), 1)
    i = np.arange(n)[:, None]
    j = np.arange(n)[None, :]
    jj = np.maximum(i, j)
    J = K1[jj + 1] - K1[i] - (K2[jj + 1, jj + 1] + K2[i, i] - K2[jj + 1, i] - K2[i, jj + 1]) / (jj - i + 1)
    return np.where(j >= i, J, 0.0)


def dp(J, m, lmin=1, lmax=100000):
    """(I [m + 1, n + 1], p [m + 1, n + 1]) of the dynamic program over the scatter table J; each step k is one masked
    [n, n] reduction (rows: segment end l - 1, columns: split t; np.argmin keeps the first, i.e. smallest, t)."""
    n = J.shape[0]
    I = np.full((m + 1, n + 1), 1e101)
    p = np.zeros((m + 1, n + 1), dtype=np.int64)
    hi = min(lmax, n + 1)
    if hi > lmin:
        I[0, lmin:hi] = J[0, lmin - 1:hi - 1]
    if m == 0:
        return I, p
    JT = np.ascontiguousarray(J.T)                      # JT[e, t] = J[t, e]
    l = np.arange(1, n + 1)[:, None]
    t = np.arange(n)[None, :]
    window = (t <= l - lmin) & (t >= l - lmax)
    C = np.empty((n, n))
    for k in range(1, m + 1):
        np.add(I[k - 1, :n][None, :], JT, out=C)
        C[~(window & (t >= k * lmin))] = np.inf
        a = np.argmin(C, axis=1)
        v = C[np.arange(n), a]
        live = np.arange(1, n + 1) >= (k + 1) * lmin
        take = live & (v < 1e100)
        I[k, 1:] = np.where(take, v, np.where(live, 1e100, 1e101))
        p[k, 1:] = np.where(take, a, 0)
    return I, p


def backtrack(p, m, n):
    cps = np.zeros(m, dtype=np.int64)
    cur = n
    for k in range(m, 0, -1):
        cur = p[k, cur]
        cps[k - 1] = cur
    return cps


def cpd_nonlin(K, ncp, lmin=1, lmax=100000, backtrack_=True):
    J = scatters(K)
    n = J.shape[0]
    I, p = dp(J, ncp, lmin, lmax)
    scores = I[:, n].copy()
    scores[scores > 1e99] = np.inf
    cps = backtrack(p, ncp, n) if backtrack_ else np.zeros(ncp, dtype=np.int64)
    return cps, scores, I, p


def penalties(n, m, vmax, desc_rate=1):
    N2 = n * desc_rate
    pen = np.zeros(m + 1)
    c = np.arange(1, m + 1)
    pen[1:] = (vmax * c / (2.0 * N2)) * (np.log(float(N2) / c) + 1)
    return pen


def kts_segmentation(K, ncp, vmax, desc_rate=1, lmin=1, lmax=100000):
    """(cps, costs, scores, runner-up margin): the margin is the gap between the best and the second-best cost, the
    room within which a perturbed objective may legitimately choose another number of change points."""
    n = np.asarray(K).shape[0]
    _, scores, I, p = cpd_nonlin(K, ncp, lmin, lmax, backtrack_=False)
    costs = scores / float(n) + penalties(n, ncp, vmax, desc_rate)
    m_best = int(np.argmin(costs))
    srt = np.sort(costs)
    margin = float(srt[1] - srt[0]) if len(srt) > 1 else np.inf
    return backtrack(p, m_best, n), costs, scores, margin


def objective(K, cps):
    """sum of the segments' scatters for the given change points (float64)."""
    J = scatters(K)
    b = [0] + [int(c) for c in cps] + [J.shape[0]]
    return float(sum(J[b[i], b[i + 1] - 1] for i in range(len(b) - 1)))


def planted(n, D, n_shots, seed, noise=0.5):
    """piecewise-constant centroids plus noise, L2-normalised rows (float32)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cuts = np.sort(rng.choice(np.arange(8, n - 8), size=n_shots - 1, replace=False))
    lab = np.searchsorted(cuts, np.arange(n), side="right")
    cent = rng.standard_normal((n_shots, D))
    x = cent[lab] + noise * rng.standard_normal((n, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def planted_int(n, D, n_shots, seed, amp=2, noise=1):
    """piecewise-constant integer centroids in [-amp, amp] plus integer noise in [-noise, noise] (float32 [n, D]): inputs
    on which the Gram, the prefix sums, the scatter table and the dynamic program are exact in every summation order
    (assert_exact).  Cuts come from 1..n-1, n_shots is clamped to n; noise = 0 with one shot gives identical frames."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_shots = max(1, min(int(n_shots), n))
    cuts = np.sort(rng.choice(np.arange(1, n), size=n_shots - 1, replace=False))
    lab = np.searchsorted(cuts, np.arange(n), side="right")
    cent = rng.integers(-amp, amp + 1, size=(n_shots, D))
    x = cent[lab] + rng.integers(-noise, noise + 1, size=(n, D))
    return x.astype(np.float32)


def assert_exact(x):
    """The premise of the bit-equality tests, checked: the float32 Gram of x equals the float64 one (every partial sum an
    integer below 2^24), and the prefix sums of K stay integers below 2^53.  Returns K = X X^T in float64."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and (x == np.rint(x)).all()
    x64 = x.astype(np.float64)
    K = x64 @ x64.T
    assert np.array_equal(np.dot(x, x.T).astype(np.float64), K)
    assert (np.abs(x64).sum(1).max() * np.abs(x64).max()) < 2.0 ** 24      # every partial sum of a dot product too
    assert np.abs(K).max() < 2.0 ** 24 and np.abs(K).sum() < 2.0 ** 53
    return K


def unstructured(n, D, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((n, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def rbf(x, gamma):
    x = np.asarray(x, dtype=np.float64)
    sq = (x * x).sum(1)
    return np.exp(-gamma * np.maximum(sq[:, None] + sq[None, :] - 2.0 * x @ x.T, 0.0))
