"""GPU: kernel temporal segmentation on the MI355X against the reference's goldens and the float64 restatement."""
import importlib
import io
import contextlib

import numpy as np
import pytest
import torch

import kts_ref
from test_kts_host import CASES, case_kernel, exact_case, golden, rel

pytestmark = pytest.mark.gpu

# the GPU's fp32 Gram (float64 everything after it) against the restatement on float64 features
REL_RESTATED = 1e-6


@pytest.fixture(scope="module")
def seg():
    return importlib.import_module("video-summarization_amd").segmentation


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_golden_case(seg, name):
    c, z = CASES[name], golden()[1]
    x, K = case_kernel(c)
    exact = exact_case(c)                  # integer inputs (kts_ref.assert_exact): bit-equal to the reference
    if exact:
        kts_ref.assert_exact(x)
    with contextlib.redirect_stdout(io.StringIO()):
        if c["fn"] == "kts_seg":
            cps = seg.kts_seg(x, c["ncp"], c["vmax"])                    # features in: the Gram on the GPU
            _, vals = seg.kts_segmentation(K, c["ncp"], c["vmax"])       # the costs of the same call through K
        elif c["fn"] == "kts_segmentation":
            kw = {k: c[k] for k in ("lmin", "lmax") if k in c}
            cps, vals = seg.kts_segmentation(torch.from_numpy(np.asarray(K)).cuda(), c["ncp"], c["vmax"], c.get("desc_rate", 1), **kw)
        else:
            kw = {k: c[k] for k in ("lmin", "lmax") if k in c}
            sc = [None] if c.get("out_scatters") else None
            cps, vals = seg.cpd_nonlin(K, c["ncp"], backtrack=c["backtrack"], out_scatters=sc, **kw)
            if sc is not None:
                g = z[name + "/scatters"]
                assert sc[0].shape == g.shape and sc[0].dtype == np.float64
                assert (np.tril(sc[0], -1) == 0).all()
                if exact:
                    np.testing.assert_array_equal(sc[0], g)
                else:
                    assert np.abs(sc[0] - g).max() <= 5e-5 * np.abs(g).max()
    assert cps.dtype == np.int64 and vals.dtype == np.float64
    np.testing.assert_array_equal(cps, z[name + "/cps"])
    if exact and c["fn"] == "cpd_nonlin":
        np.testing.assert_array_equal(vals, z[name + "/vals"])
    else:
        assert rel(vals, z[name + "/vals"]) <= (1e-12 if exact else 5e-5)     # exact scores, then a log in the penalty


def _restated_check(seg, x, ncp, vmax):
    x64 = x.astype(np.float64)
    K64 = x64 @ x64.T
    ref_cps, ref_costs, ref_scores, margin = kts_ref.kts_segmentation(K64, ncp, vmax)
    cps = seg.kts_seg(x, ncp, vmax)
    with contextlib.redirect_stdout(io.StringIO()):
        _, costs = seg.kts_segmentation(np.dot(x, x.T), ncp, vmax, verbose=False)
    err = rel(costs, ref_costs)
    assert err <= REL_RESTATED, err
    if margin > 2 * REL_RESTATED * np.abs(ref_costs).max():
        np.testing.assert_array_equal(cps, ref_cps)
    else:                                            # an honest near-tie: the chosen split is optimal in float64 too
        got = kts_ref.objective(K64, cps) / len(x) + kts_ref.penalties(len(x), ncp, vmax)[len(cps)]
        assert abs(got - ref_costs.min()) <= REL_RESTATED * abs(ref_costs.min())
    return cps, ref_cps


@pytest.mark.parametrize("n,D,shots,ncp,seed", [(300, 1024, 10, 30, 31), (700, 512, 20, 70, 32), (1000, 1024, 25, 100, 33),
                                                 (2000, 1024, 40, 200, 34)])
def test_planted_against_the_float64_restatement(seg, n, D, shots, ncp, seed):
    cps, ref = _restated_check(seg, kts_ref.planted(n, D, shots, seed), ncp, 1.0)
    np.testing.assert_array_equal(cps, ref)                 # planted shots: far above the margin bound


@pytest.mark.parametrize("n,ncp,seed", [(500, 50, 41), (1200, 60, 42)])
def test_unstructured_against_the_float64_restatement(seg, n, ncp, seed):
    _restated_check(seg, kts_ref.unstructured(n, 512, seed), ncp, 0.05)


def test_ncp_n_minus_1_against_the_float64_restatement(seg):
    _restated_check(seg, kts_ref.planted(400, 512, 12, 43), 399, 1.0)


def test_cpd_nonlin_backtrack_matches_the_restatement_on_every_row(seg):
    x = kts_ref.planted(600, 512, 15, 44)
    K = x.astype(np.float64) @ x.astype(np.float64).T              # float64 K: no fp32 rounding anywhere
    for lmin, lmax in ((1, 100000), (4, 90)):
        cps, scores = seg.cpd_nonlin(K, 30, lmin, lmax, verbose=False)
        rcps, rscores, _, _ = kts_ref.cpd_nonlin(K, 30, lmin, lmax)
        np.testing.assert_array_equal(cps, rcps)
        assert rel(scores, rscores) <= 1e-12


def test_batch_is_bitwise_equal_to_single_calls_and_deterministic(seg):
    tools = importlib.import_module("tools.eval_corpus")
    feats, _, _ = tools.corpus()
    feats = [f.cuda() for f in feats]
    ncp = [max(1, len(f) // 10) for f in feats]
    a = seg.kts_seg_batch(feats, ncp, 1.0)
    b = seg.kts_seg_batch(feats, ncp, 1.0)
    assert len(a) == 75
    for f, m, ca, cb in zip(feats, ncp, a, b):
        np.testing.assert_array_equal(ca, cb)
        np.testing.assert_array_equal(ca, seg.kts_seg(f, m, 1.0))
    # costs bitwise too (the scores path of one video vs the batch)
    lengths = [len(f) for f in feats[:5]]
    Ks = torch.cat([(f @ f.T).reshape(-1) for f in feats[:5]])
    _, batch_costs = seg._segment(Ks, 1, lengths, ncp[:5], 2, vmax=[1.0] * 5)
    for i in range(5):
        _, one = seg._segment((feats[i] @ feats[i].T).reshape(-1), 1, lengths[i:i + 1], ncp[i:i + 1], 2, vmax=[1.0])
        assert np.array_equal(batch_costs[i], one[0])


def test_end_to_end_score_shots_summary(seg):
    vsa = importlib.import_module("video-summarization_amd")
    ev = importlib.import_module("video-summarization_amd.evaluation")
    T, nf = 240, 240 * 15
    x = kts_ref.planted(T, 1024, 9, 51)
    picks = np.arange(0, nf, 15)
    m = vsa.SimNet(num_heads=4, d_model=256, num_layers=4, sparsity=0.0, dropout=0.3)
    m.load_state_dict(vsa.synth.make_state_dict(256, 4, 1234))
    m = m.cuda().eval()
    with torch.no_grad():
        scores = m.score(torch.from_numpy(x).cuda()[None]).reshape(-1).float().cpu().numpy()
    cps = seg.kts_seg(x, 24, 1.0)
    x64 = x.astype(np.float64)
    rcps = kts_ref.kts_segmentation(x64 @ x64.T, 24, 1.0)[0]
    np.testing.assert_array_equal(cps, rcps)
    shots = seg.shots_from_change_points(cps, nf, picks)
    rshots = seg.shots_from_change_points(rcps, nf, picks)
    s = ev.generate_summary([shots], [scores], [nf], [picks])[0]
    r = ev.generate_summary([rshots], [scores], [nf], [picks])[0]
    np.testing.assert_array_equal(s, r)
    assert s.sum() > 0


def test_inputs_on_cpu_and_gpu_numpy_and_torch_agree(seg):
    x = kts_ref.planted(150, 512, 5, 52)
    a = seg.kts_seg(x, 15, 1.0)
    b = seg.kts_seg(torch.from_numpy(x), 15, 1.0)
    c = seg.kts_seg(torch.from_numpy(x).cuda(), 15, 1.0)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)
    # a feature width that is not a multiple of 32 (zero-padded for the GEMM)
    y = np.ascontiguousarray(x[:, :100])
    y64 = y.astype(np.float64)
    np.testing.assert_array_equal(seg.kts_seg(y, 15, 1.0), kts_ref.kts_segmentation(y64 @ y64.T, 15, 1.0)[0])
