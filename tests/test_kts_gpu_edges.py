"""GPU: kernel temporal segmentation bit for bit at tile, chunk and window edges.

Every input here is integer valued (kts_ref.planted_int, or an integer kernel matrix built from it), and on such inputs
every stage of csrc/vs_segment.hip is exact or order-identical to the float64 restatement tests/kts_ref.py:
  Gram      entries in [-3, 3], D <= 1024: every partial sum of a dot product is an integer below 2^24, so the fp32 MFMA
            Gram has the same bits in any summation order and in either GEMM family;
  prefixes  K1 and K2 are integers far below 2^53: block scans, chunked column scans and numpy's cumsum agree;
  scatter   kts_scatter evaluates (K1[e+1] - K1[s]) - (((K2ee + K2ss) - K2es) - K2se) / len in the order of
            kts_ref.scatters, contraction off, no fast-math: one correctly rounded divide and subtract on both sides;
  DP        a step is one fp64 add and compares, ties to the smallest t on both sides.
So the bar is np.array_equal on the scatter table, the scores (+inf positions included) and the change points, not a
tolerance; every test first asserts the premise on its input (kts_ref.assert_exact).  The one exception is the cost
vector of VS_KTS_AUTO: its penalty passes through log, where libm and numpy may differ by an ulp, so costs are held to
1e-12 relative (the bar of test_cpd_nonlin_backtrack_matches_the_restatement_on_every_row) while m_best and the change
points must be equal; every AUTO comparison asserts on the CPU side that the runner-up is further than 1e-9 away.

The sizes are the strides of the kernels: 32 x 32 tiles (kts_scatter, kts_scatters_out), 64-row chunks (kts_colsum,
kts_colapply), 256 columns per block over n + 1 columns, 4 segment ends per block and a 64-lane window with an x4
unroll (kts_dp_step), 1024 columns per pass of the row scan, round32(n) rows and round32(D) columns of the Gram.
"""
import functools
import importlib

import numpy as np
import pytest
import torch

import kts_ref
from test_kts_host import rel

pytestmark = pytest.mark.gpu

vsa = importlib.import_module("video-summarization_amd")
seg, L = vsa.segmentation, vsa._lib
FEATS, KF32, KF64 = L.VS_KTS_FEATURES_F32, L.VS_KTS_KERNEL_F32, L.VS_KTS_KERNEL_F64
SCORES, BACKTRACK, AUTO = L.VS_KTS_SCORES, L.VS_KTS_BACKTRACK, L.VS_KTS_AUTO
LMAX = 100000
REL_COSTS = 1e-12          # AUTO costs only (log in the penalty); everything else is array_equal
MARGIN = 1e-9              # runner-up distance, relative to max|costs|, below which m_best would be a coin toss


def cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()         # a copy: the shared references stay read-only


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def video(n, D, shots, seed, amp=2, noise=1):
    """(x float32 [n, D], K = X X^T float64), the exactness premise asserted; shared and read-only."""
    x = kts_ref.planted_int(n, D, shots, seed, amp, noise)
    return frozen(x, kts_ref.assert_exact(x))


@functools.lru_cache(maxsize=None)
def table(n, D, shots, seed, amp=2, noise=1):
    return frozen(kts_ref.scatters(video(n, D, shots, seed, amp, noise)[1]))[0]


@functools.lru_cache(maxsize=None)
def restated(n, D, shots, seed, m, lmin=1, lmax=LMAX, amp=2, noise=1):
    """(cps, scores, I, p) of kts_ref on that video."""
    I, p = kts_ref.dp(table(n, D, shots, seed, amp, noise), m, lmin, lmax)
    scores = I[:, n].copy()
    scores[scores > 1e99] = np.inf
    return frozen(kts_ref.backtrack(p, m, n), scores, I, p)


def auto_restated(K, m, vmax, desc_rate=1, lmin=1, lmax=LMAX):
    """kts_ref.kts_segmentation with the margin condition asserted: (cps, costs)."""
    cps, costs, _, margin = kts_ref.kts_segmentation(K, m, vmax, desc_rate, lmin, lmax)
    finite = costs[np.isfinite(costs)]
    assert finite.size and margin > MARGIN * np.abs(finite).max(), (margin, costs)
    return cps, costs


def equal(a, b):
    np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# a. the scatter table at tile and chunk edges, from all three input kinds

A_SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025]


def a_video(n):
    return (n, 128, n // 50 + 2, 100 + n)


@pytest.mark.parametrize("n", A_SIZES)
def test_scatter_table_is_bit_equal_from_features_float32_and_float64_kernels(n):
    x, K = video(*a_video(n))
    J = table(*a_video(n))
    for kind, t in ((FEATS, cuda(x)), (KF32, cuda(K.astype(np.float32))), (KF64, cuda(K))):
        got = seg._scatters(t, kind, n)
        assert got.shape == (n, n) and got.dtype == np.float64
        equal(got, J)                                   # the zeros below the diagonal included
    sc = [None]
    seg.cpd_nonlin(cuda(K), 0, verbose=False, out_scatters=sc)
    equal(sc[0], J)


@pytest.mark.parametrize("n", [33, 257])
def test_scatters_writes_nothing_past_its_output_or_its_workspace(n):
    x, _ = video(*a_video(n))
    lib, t = L.load(), cuda(x)
    cu, zero = seg._i32([0, n]), seg._i32([0])
    nbytes = lib.vs_kts_workspace_bytes(seg._p(cu), 1, x.shape[1], FEATS, seg._p(zero), SCORES)
    assert nbytes > 0
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    sentinel = -7.25e300
    out = torch.full((n * n + 64,), sentinel, dtype=torch.float64, device="cuda")
    L.check(lib.vs_kts_scatters(t.data_ptr(), FEATS, x.shape[1], n, out.data_ptr(), ws.data_ptr(), nbytes,
                                torch.cuda.current_stream().cuda_stream))
    o = out.cpu().numpy()
    assert (o[n * n:] == sentinel).all()
    equal(o[:n * n].reshape(n, n), table(*a_video(n)))
    assert (ws[nbytes:] == 0xA5).all().item()


# ---------------------------------------------------------------------------------------------------------------------
# b. the Gram at feature-width and GEMM-family edges

@pytest.fixture
def gemm_family():
    """pin(True): VS_SKINNY_ROWS=0, the LDS-tiled GEMM with N = round32(n); pin(False): the default choice."""
    def pin(tiled):
        L.set_option("VS_SKINNY_ROWS", 0 if tiled else -1)
    yield pin
    L.set_option("VS_SKINNY_ROWS", -1)


@pytest.mark.parametrize("n", [1, 33, 129, 257])
@pytest.mark.parametrize("D", [1, 7, 31, 32, 33, 96, 100, 128, 160, 1024])
def test_gram_at_feature_width_and_gemm_family_edges(gemm_family, D, n):
    v = (n, D, 4, 1000 * D + n)
    x, _ = video(*v)
    m = min(n - 1, 7)
    J = table(*v)
    rcps, rscores, _, _ = restated(*v, m)
    got = []
    for tiled in (False, True):
        gemm_family(tiled)
        t = cuda(x)
        Jg = seg._scatters(t, FEATS, n)
        cps, scores = seg._segment(t, FEATS, [n], [m], BACKTRACK)
        equal(Jg, J)
        equal(scores[0], rscores)
        equal(cps[0], rcps)
        got.append((Jg, scores[0], cps[0]))
    for a, b in zip(*got):                              # the two GEMM families: the same bits as each other
        equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# c. the dynamic program of one video: window, unroll, constraints, unreachable entries

def c_video(n):
    return (n, 48, n // 40 + 2, 200 + n)


DP_CASES = [(513, 12, 1, LMAX), (1025, 8, 1, LMAX), (513, 12, 5, 300), (258, 12, 5, 60),
            (65, 64, 1, LMAX),                       # ncp = n - 1
            (60, 5, 10, 10),                         # I[0, lmin:lmax] is empty: every score +inf
            (60, 5, 2, 12),                          # every score but the last +inf
            (1, 0, 1, LMAX), (2, 1, 1, LMAX),
            (129, 10, 2, 2 ** 31 - 1)]


@pytest.mark.parametrize("n,ncp,lmin,lmax", DP_CASES)
def test_cpd_nonlin_is_bit_equal_with_and_without_backtrack(n, ncp, lmin, lmax):
    _, K = video(*c_video(n))
    rcps, rscores, _, _ = restated(*c_video(n), ncp, lmin, lmax)
    cps, scores = seg.cpd_nonlin(cuda(K), ncp, lmin, lmax, verbose=False)
    assert cps.dtype == np.int64 and scores.dtype == np.float64
    equal(scores, rscores)                              # +inf positions included
    equal(cps, rcps)
    cps0, scores0 = seg.cpd_nonlin(cuda(K), ncp, lmin, lmax, backtrack=False, verbose=False)
    equal(scores0, rscores)
    equal(cps0, np.zeros(ncp, dtype=np.int64))
    if (n, lmin, lmax) == (60, 10, 10):
        assert np.isinf(rscores).all()
    if (n, lmin, lmax) == (60, 2, 12):
        assert np.isinf(rscores[:-1]).all() and np.isfinite(rscores[-1])


# (n, ncp, lmin, lmax, vmax, desc_rate): vmax is on the scale of these un-normalised integer features (vmax = 1.0
# always selects ncp), chosen so that the restatement's m_best is interior; asserted below, not assumed
AUTO_CASES = [(513, 12, 1, LMAX, 1000.0, 1), (513, 12, 5, 300, 1000.0, 1), (258, 12, 5, 60, 1000.0, 1),
              (513, 12, 1, LMAX, 8000.0, 15)]


@pytest.mark.parametrize("n,ncp,lmin,lmax,vmax,desc_rate", AUTO_CASES)
def test_kts_segmentation_selects_the_restatements_interior_m_best(n, ncp, lmin, lmax, vmax, desc_rate):
    _, K = video(*c_video(n))
    rcps, rcosts = auto_restated(K, ncp, vmax, desc_rate, lmin, lmax)
    assert 0 < len(rcps) < ncp, len(rcps)
    cps, costs = seg.kts_segmentation(cuda(K), ncp, vmax, desc_rate, lmin=lmin, lmax=lmax, verbose=False)
    assert rel(costs, rcosts) <= REL_COSTS
    equal(cps, rcps)


# ---------------------------------------------------------------------------------------------------------------------
# d. the whole DP table through a batch of prefixes: I[k, l] of the full problem is the final score k of the problem on
# the first l frames, so one batched call returns every column of I - entries off the optimal path included

def prefix_batch(v, m, lmin, lmax, ls):
    n = v[0]
    _, K = video(*v)
    _, _, I, p = restated(*v, m, lmin, lmax)
    jobs = [(l, min(m, l // lmin - 1)) for l in ls]
    jobs = [(l, ml) for l, ml in jobs if l <= (ml + 1) * lmax]            # the reference's n <= (ncp + 1) lmax
    assert jobs and max(l for l, _ in jobs) <= n
    Ks = cuda(np.concatenate([K[:l, :l].ravel() for l, _ in jobs]))
    lens, ncps = [l for l, _ in jobs], [ml for _, ml in jobs]
    B = len(jobs)
    cps_b, sc_b = seg._segment(Ks, KF64, lens, ncps, BACKTRACK, [lmin] * B, [lmax] * B)
    cps_s, sc_s = seg._segment(Ks, KF64, lens, ncps, SCORES, [lmin] * B, [lmax] * B)
    for i, (l, ml) in enumerate(jobs):
        col = I[:ml + 1, l].copy()
        col[col > 1e99] = np.inf
        equal(sc_b[i], col)
        equal(cps_b[i], kts_ref.backtrack(p, ml, l))    # p of the full problem, walked from the prefix's end
        equal(sc_s[i], col)
        equal(cps_s[i], np.zeros(ml, dtype=np.int64))
    return len(jobs)


@pytest.mark.parametrize("m,lmin,lmax", [(6, 1, LMAX), (6, 3, 40)])
def test_every_entry_of_the_dp_table_through_a_batch_of_prefixes(m, lmin, lmax):
    n = 160
    assert prefix_batch((n, 24, 6, 301), m, lmin, lmax, range(lmin, n + 1)) == n - lmin + 1


def test_dp_table_columns_at_the_unroll_edges():
    # window lengths l - k around 448 = 256 + 192 and 512: the last x4 pass and the tail loop of kts_dp_step
    assert prefix_batch((530, 16, 9, 302), 8, 1, LMAX, list(range(440, 460)) + list(range(510, 530))) == 40


# ---------------------------------------------------------------------------------------------------------------------
# e. exact ties: every candidate of every step costs the same, so only the tie-break decides

TIE_PARAMS = [(6, 3, 20), (12, 1, LMAX), (5, 1, 64), (4, 1, 65)]


@pytest.mark.parametrize("ncp,lmin,lmax", TIE_PARAMS)
@pytest.mark.parametrize("n", [70, 300])
def test_identical_frames_tie_to_the_smallest_split(n, ncp, lmin, lmax):
    v = (n, 40, 1, 400 + n, 2, 0)
    x, K = video(*v)
    assert (x == x[0]).all() and x.any()
    assert not table(*v).any()                          # J == 0 everywhere
    if n > (ncp + 1) * lmax:                            # (300, 6, 3, 20): the reference's assert, a refusal here
        with pytest.raises(ValueError):
            seg.cpd_nonlin(cuda(K), ncp, lmin, lmax, verbose=False)
        return
    rcps, rscores, _, _ = restated(*v[:4], ncp, lmin, lmax, *v[4:])
    assert not rscores[np.isfinite(rscores)].any() and np.isfinite(rscores[-1])
    cps, scores = seg.cpd_nonlin(cuda(K), ncp, lmin, lmax, verbose=False)
    equal(scores, rscores)
    equal(cps, rcps)
    if lmax >= n:                                       # unconstrained closed form: the smallest feasible t is k lmin
        equal(cps, lmin * np.arange(1, ncp + 1))
    fcps, fscores = seg._segment(cuda(x), FEATS, [n], [ncp], BACKTRACK, [lmin], [lmax])
    equal(fscores[0], rscores)
    equal(fcps[0], rcps)


def test_block_diagonal_kernel_ties_inside_its_shots():
    # three shots of identical frames with orthogonal centroids: K is block diagonal, the three-shot split costs 0 and
    # every further change point is a tie among all positions
    lens, D = (30, 34, 33), 8
    x = np.zeros((sum(lens), D), dtype=np.float32)
    at = 0
    for i, ln in enumerate(lens):
        x[at:at + ln, 2 * i] = i + 1
        x[at:at + ln, 2 * i + 1] = -2
        at += ln
    K = kts_ref.assert_exact(x)
    n = len(x)
    assert not K[:30, 30:].any() and not K[30:64, 64:].any()
    for ncp, lmin, lmax in ((6, 1, LMAX), (9, 2, 40), (5, 1, 64)):
        rcps, rscores, _, _ = kts_ref.cpd_nonlin(K, ncp, lmin, lmax)
        assert not rscores[2:][np.isfinite(rscores[2:])].any() and rscores[-1] == 0
        for t in (K, K.astype(np.float32)):
            cps, scores = seg.cpd_nonlin(cuda(t), ncp, lmin, lmax, verbose=False)
            equal(scores, rscores)
            equal(cps, rcps)
        fcps, fscores = seg._segment(cuda(x), FEATS, [n], [ncp], BACKTRACK, [lmin], [lmax])
        equal(fscores[0], rscores)
        equal(fcps[0], rcps)


# ---------------------------------------------------------------------------------------------------------------------
# f. ragged batches with per-video parameters (a long video before a short one: the shared xpad buffer is reused)

F_LEN = [300, 33, 1, 129, 64, 257, 2]
F_NCP = [20, 3, 0, 12, 7, 9, 1]
F_LMIN = [1, 2, 1, 4, 1, 3, 1]
F_LMAX = [LMAX, 15, LMAX, 30, 64, 100, LMAX]
F_VMAX = [1500.0, 800.0, 1.0, 1500.0, 800.0, 3000.0, 50.0]


def f_videos(D):
    return [(n, D, n // 30 + 2, 500 + 7 * D + n) for n in F_LEN]


def f_batch(D, order, mode):
    xs = [video(*f_videos(D)[i])[0] for i in order]
    pick = lambda v: [v[i] for i in order]
    return seg._segment(cuda(np.concatenate(xs)), FEATS, pick(F_LEN), pick(F_NCP), mode, pick(F_LMIN), pick(F_LMAX),
                        pick(F_VMAX) if mode == AUTO else None)


@pytest.mark.parametrize("mode", [SCORES, BACKTRACK, AUTO])
@pytest.mark.parametrize("D", [100, 128])               # the two xpad zeroing branches: d != d_pad, d == d_pad
def test_ragged_batch_with_per_video_parameters(D, mode):
    B = len(F_LEN)
    fwd = list(range(B))
    cps, vals = f_batch(D, fwd, mode)
    cps2, vals2 = f_batch(D, fwd, mode)
    rev = fwd[::-1]
    cps_r, vals_r = f_batch(D, rev, mode)
    for i in range(B):
        v, n, m, lo, hi = f_videos(D)[i], F_LEN[i], F_NCP[i], F_LMIN[i], F_LMAX[i]
        x, K = video(*v)
        if mode == AUTO:
            rcps, rvals = auto_restated(K, m, F_VMAX[i], 1, lo, hi)
            assert rel(vals[i], rvals) <= REL_COSTS
        else:
            rcps, rvals, _, _ = restated(*v, m, lo, hi)
            if mode == SCORES:
                rcps = np.zeros(m, dtype=np.int64)
            equal(vals[i], rvals)
        equal(cps[i], rcps)
        one_c, one_v = seg._segment(cuda(x), FEATS, [n], [m], mode, [lo], [hi], [F_VMAX[i]] if mode == AUTO else None)
        equal(cps[i], one_c[0])                         # the batch against the single-video call, costs bit for bit
        equal(vals[i], one_v[0])
        equal(cps[i], cps2[i])                          # run to run
        equal(vals[i], vals2[i])
        equal(cps[i], cps_r[B - 1 - i])                 # and whatever the video's place in the batch
        equal(vals[i], vals_r[B - 1 - i])


@pytest.mark.parametrize("D", [100, 128])
def test_kts_seg_batch_takes_per_video_num_seg_v_max_lmin_lmax(D):
    xs = [cuda(video(*v)[0]) for v in f_videos(D)]
    got = seg.kts_seg_batch(xs, F_NCP, F_VMAX, F_LMIN, F_LMAX)
    assert len(got) == len(F_LEN)
    for i, v in enumerate(f_videos(D)):
        rcps, _ = auto_restated(video(*v)[1], F_NCP[i], F_VMAX[i], 1, F_LMIN[i], F_LMAX[i])
        assert got[i].dtype == np.int64
        equal(got[i], rcps)


# ---------------------------------------------------------------------------------------------------------------------
# g. workspace and output bounds: guard bands around everything vs_kts_segment writes

@pytest.mark.parametrize("kind", [FEATS, KF64])
def test_segment_writes_nothing_past_its_workspace_or_its_host_outputs(kind):
    D, B, guard, pad = 100, len(F_LEN), 4096, 16
    vids = [video(*v) for v in f_videos(D)]
    if kind == FEATS:
        t, d = cuda(np.concatenate([x for x, _ in vids])), D
    else:
        t, d = cuda(np.concatenate([K.ravel() for _, K in vids])), 0
    lib = L.load()
    cu = seg._i32(np.concatenate([[0], np.cumsum(F_LEN)]))
    ncp, lmin, lmax, vmax = seg._i32(F_NCP), seg._i32(F_LMIN), seg._i32(F_LMAX), seg._f64(F_VMAX)
    nbytes = lib.vs_kts_workspace_bytes(seg._p(cu), B, d, kind, seg._p(ncp), AUTO)
    assert nbytes > 0
    buf = torch.full((guard + nbytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    n_c, n_s = int(ncp.sum()), int(ncp.sum()) + B
    cps = np.full(n_c + pad, -77, dtype=np.int64)
    n_cps = np.full(B + pad, -77, dtype=np.int32)
    vals = np.full(n_s + pad, -7.25e300, dtype=np.float64)
    L.check(lib.vs_kts_segment(t.data_ptr(), kind, d, seg._p(cu), B, seg._p(ncp), seg._p(lmin), seg._p(lmax), seg._p(vmax),
                               None, AUTO, seg._p(cps), seg._p(n_cps), seg._p(vals), buf.data_ptr() + guard, nbytes,
                               torch.cuda.current_stream().cuda_stream))
    assert (buf[:guard] == 0xA5).all().item() and (buf[guard + nbytes:] == 0xA5).all().item()
    assert (cps[n_c:] == -77).all() and (n_cps[B:] == -77).all() and (vals[n_s:] == -7.25e300).all()
    ci = si = 0
    for i, (_, K) in enumerate(vids):                   # and what it wrote inside is the answer
        m = F_NCP[i]
        rcps, rcosts = auto_restated(K, m, F_VMAX[i], 1, F_LMIN[i], F_LMAX[i])
        assert n_cps[i] == len(rcps)
        equal(cps[ci:ci + n_cps[i]], rcps)
        equal(cps[ci + n_cps[i]:ci + m], np.zeros(m - n_cps[i], dtype=np.int64))
        assert rel(vals[si:si + m + 1], rcosts) <= REL_COSTS
        ci += m
        si += m + 1
