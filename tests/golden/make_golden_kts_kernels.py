"""Writes tests/golden/kts_kernels_golden.npz: the reference's kts_segmentation / eval_score / estimate_vmax (numpy only)
on the float64 cosine and rbf kernel matrices of planted-shot features (tests/kts_kernels_ref.py).  Data only: the
float32 features, each case's kernel and parameters, and the reference's results.

    python tests/golden/make_golden_kts_kernels.py --reference <checkout of the reference>/src/data/preprocess/segmentations

Per case the script also runs the reference on the kernel whose Gram was accumulated in float32 (numpy) and asserts the
conditions that make the golden a fair target for an fp32-Gram implementation:
    the change points of both kernels are identical,
    margin (best to second-best cost) >= 1000 x cost_err32 (max |costs32 - costs64|),
    0 < m_best < ncp.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kts_kernels_ref as kk  # noqa: E402

NCP = 15
# feature sets: shot lengths, D, noise, seed
FEATURES = {
    "six_d64": dict(lengths=[20, 33, 17, 40, 25, 15], D=64, noise=0.3, seed=101),
    "seven_d100": dict(lengths=[5, 60, 31, 32, 33, 9, 30], D=100, noise=0.5, seed=103),
    "four_d32": dict(lengths=[64, 64, 65, 63], D=32, noise=0.4, seed=101),
}
# kernel cases: gamma as a multiple of 1 / D (None for cosine), vmax
CASES = {
    "six_d64/cosine": dict(x="six_d64", kind="cosine", gamma_d=None, vmax=0.1),
    "six_d64/rbf_1": dict(x="six_d64", kind="rbf", gamma_d=1.0, vmax=0.3),
    "six_d64/rbf_025": dict(x="six_d64", kind="rbf", gamma_d=0.25, vmax=0.1),
    "seven_d100/cosine": dict(x="seven_d100", kind="cosine", gamma_d=None, vmax=0.1),
    "seven_d100/rbf_025": dict(x="seven_d100", kind="rbf", gamma_d=0.25, vmax=0.1),
    "four_d32/cosine": dict(x="four_d32", kind="cosine", gamma_d=None, vmax=0.1),
    "four_d32/rbf_1": dict(x="four_d32", kind="rbf", gamma_d=1.0, vmax=0.3),
    "four_d32/rbf_025": dict(x="four_d32", kind="rbf", gamma_d=0.25, vmax=0.1),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's segmentations directory (holds kts/)")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from kts import kts_segmentation  # noqa: the reference package, numpy only
    from kts.cpd_auto import estimate_vmax, eval_score  # noqa

    def run(K, vmax):
        with contextlib.redirect_stdout(io.StringIO()):
            cps, costs = kts_segmentation(K, NCP, vmax)
        return np.asarray(cps, dtype=np.int64), np.asarray(costs, dtype=np.float64)

    out = {}
    feats = {}
    for name, f in FEATURES.items():
        feats[name] = kk.planted_shots(f["lengths"], f["D"], f["noise"], f["seed"])
        out["x/" + name] = feats[name]
    meta = {}
    for name, c in CASES.items():
        x, f = feats[c["x"]], FEATURES[c["x"]]
        gamma = None if c["gamma_d"] is None else c["gamma_d"] / f["D"]
        K64 = kk.kernel64(x, c["kind"], gamma)
        K32 = kk.kernel64(x, c["kind"], gamma, gram32=True)
        cps, costs = run(K64, c["vmax"])
        cps32, costs32 = run(K32, c["vmax"])
        err32 = float(np.abs(costs32 - costs).max())
        srt = np.sort(costs)
        margin = float(srt[1] - srt[0])
        assert np.array_equal(cps, cps32), name
        assert margin >= 1000.0 * err32, (name, margin, err32)
        assert 0 < len(cps) < NCP, (name, len(cps))
        planted = np.cumsum(f["lengths"])[:-1]
        stable = int(f["lengths"][0])
        meta[name] = dict(x=c["x"], kind=c["kind"], gamma=gamma, ncp=NCP, vmax=c["vmax"], cost_err32=err32, margin=margin,
                          stable=stable, recovered=bool(np.array_equal(cps, planted)))
        out[name + "/cps"] = cps
        out[name + "/costs"] = costs
        out[name + "/eval_score"] = np.float64(eval_score(K64, cps))
        out[name + "/estimate_vmax"] = np.float64(estimate_vmax(K64[:stable, :stable]))
        print("%-20s m_best %2d  recovered %s  cost_err32 %.2e  margin %.2e" % (name, len(cps), meta[name]["recovered"], err32,
                                                                              margin))
    out["cases"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, "kts_kernels_golden.npz"), **out)


if __name__ == "__main__":
    main()
