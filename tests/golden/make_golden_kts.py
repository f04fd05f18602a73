"""Writes tests/golden/kts_golden.npz: the reference's kernel temporal segmentation (segmentations/kts, numpy only) on
seeded inputs.  The inputs are NOT stored: each case's recipe (tests/kts_ref.py generators + seed) is, and the tests
rebuild them bit for bit.

    python tests/golden/make_golden_kts.py --reference <checkout of the reference>/src/data/preprocess/segmentations
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
import kts_ref  # noqa: E402

# name: recipe.  fn: kts_seg (features -> K = X X^T in float32) | kts_segmentation | cpd_nonlin.
# x: ("planted", n, D, shots, seed) | ("unstructured", n, D, seed) | ("planted_int", n, D, shots, seed[, amp, noise]);
# kernel: "dot" (float32 X X^T) | ("rbf", gamma) (float64)
# The planted_int cases are exact: integer K with sum|K| < 2^24, so the reference's float32 prefix sums round nowhere
# and the tests hold them with array_equal (the costs of kts_segmentation, which pass through log, at 1e-12).
CASES = {
    "seg_planted_n60_d1024": dict(fn="kts_seg", x=("planted", 60, 1024, 4, 11), ncp=10, vmax=1.0),
    "seg_planted_n200_d1024": dict(fn="kts_seg", x=("planted", 200, 1024, 8, 12), ncp=20, vmax=1.0),
    "seg_planted_n400_d1024": dict(fn="kts_seg", x=("planted", 400, 1024, 12, 13), ncp=40, vmax=1.0),
    "seg_planted_n200_d512": dict(fn="kts_seg", x=("planted", 200, 512, 6, 14), ncp=20, vmax=1.0),
    "seg_planted_n400_d512": dict(fn="kts_seg", x=("planted", 400, 512, 10, 15), ncp=40, vmax=1.0),
    "seg_unstructured_n200_d1024": dict(fn="kts_seg", x=("unstructured", 200, 1024, 16), ncp=20, vmax=1.0),
    "seg_ncp_n_minus_1_n150": dict(fn="kts_seg", x=("planted", 150, 512, 6, 17), ncp=149, vmax=1.0),
    "auto_lmin3_lmax60_n200": dict(fn="kts_segmentation", x=("planted", 200, 512, 6, 18), kernel="dot", ncp=20, vmax=1.0,
                                   lmin=3, lmax=60),
    "auto_desc_rate15_n200": dict(fn="kts_segmentation", x=("planted", 200, 1024, 7, 19), kernel="dot", ncp=20, vmax=1.0,
                                  desc_rate=15),
    "auto_rbf_f64_n200": dict(fn="kts_segmentation", x=("planted", 200, 512, 5, 20), kernel=("rbf", 0.5), ncp=15, vmax=0.5),
    "cpd_backtrack_lmax50_n200": dict(fn="cpd_nonlin", x=("planted", 200, 512, 6, 21), kernel="dot", ncp=8, lmin=2,
                                      lmax=50, backtrack=True),
    "cpd_no_backtrack_n200": dict(fn="cpd_nonlin", x=("planted", 200, 1024, 6, 22), kernel="dot", ncp=12, backtrack=False),
    "cpd_out_scatters_n60": dict(fn="cpd_nonlin", x=("planted", 60, 1024, 3, 23), kernel="dot", ncp=5, backtrack=True,
                                 out_scatters=True),
    "int_cpd_n1_ncp0": dict(fn="cpd_nonlin", x=("planted_int", 1, 32, 1, 61), kernel="dot", ncp=0, backtrack=True),
    "int_cpd_n33": dict(fn="cpd_nonlin", x=("planted_int", 33, 32, 3, 62), kernel="dot", ncp=6, backtrack=True),
    "int_cpd_ncp_n_minus_1_n65": dict(fn="cpd_nonlin", x=("planted_int", 65, 32, 4, 63), kernel="dot", ncp=64,
                                      backtrack=True),
    "int_cpd_all_inf_n60": dict(fn="cpd_nonlin", x=("planted_int", 60, 32, 3, 64), kernel="dot", ncp=5, lmin=10, lmax=10,
                                backtrack=True),
    "int_cpd_last_score_finite_n60": dict(fn="cpd_nonlin", x=("planted_int", 60, 32, 3, 65), kernel="dot", ncp=5, lmin=2,
                                          lmax=12, backtrack=True),
    "int_cpd_all_tie_n70": dict(fn="cpd_nonlin", x=("planted_int", 70, 32, 1, 66, 2, 0), kernel="dot", ncp=6, lmin=3,
                                lmax=20, backtrack=True),
    "int_cpd_out_scatters_n33": dict(fn="cpd_nonlin", x=("planted_int", 33, 32, 3, 67), kernel="dot", ncp=5,
                                     backtrack=True, out_scatters=True),
    "int_auto_lmin2_lmax50_desc15_n120": dict(fn="kts_segmentation", x=("planted_int", 120, 32, 5, 68), kernel="dot",
                                              ncp=12, vmax=400.0, desc_rate=15, lmin=2, lmax=50),
}


def features(rec):
    if rec[0] == "planted":
        return kts_ref.planted(*rec[1:])
    if rec[0] == "planted_int":
        x = kts_ref.planted_int(*rec[1:])
        assert np.abs(kts_ref.assert_exact(x)).sum() < 2 ** 24      # the reference sums a float32 K in float32
        return x
    return kts_ref.unstructured(*rec[1:])


def kernel(x, kind):
    if kind == "dot":
        return np.dot(x, x.T)
    return kts_ref.rbf(x, kind[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's segmentations directory (holds kts/)")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from kts import cpd_nonlin, kts_segmentation  # noqa: the reference package, numpy only

    out = {"cases": np.array(json.dumps(CASES))}
    for name, c in CASES.items():
        x = features(c["x"])
        sink = io.StringIO()
        with contextlib.redirect_stdout(sink):
            if c["fn"] == "kts_seg":
                cps, vals = kts_segmentation(np.dot(x, x.T), c["ncp"], c["vmax"])
            elif c["fn"] == "kts_segmentation":
                kw = {k: c[k] for k in ("lmin", "lmax") if k in c}
                cps, vals = kts_segmentation(kernel(x, c["kernel"]), c["ncp"], c["vmax"], c.get("desc_rate", 1), **kw)
            else:
                kw = {k: c[k] for k in ("lmin", "lmax") if k in c}
                sc = [None] if c.get("out_scatters") else None
                cps, vals = cpd_nonlin(kernel(x, c["kernel"]), c["ncp"], backtrack=c["backtrack"], out_scatters=sc, **kw)
                if sc is not None:
                    out[name + "/scatters"] = np.asarray(sc[0], dtype=np.float64)
        out[name + "/cps"] = np.asarray(cps, dtype=np.int64)
        out[name + "/vals"] = np.asarray(vals, dtype=np.float64)
        print("%-30s cps %3d  vals[0] %.6g" % (name, len(cps), vals[0]))
    np.savez_compressed(os.path.join(HERE, "kts_golden.npz"), **out)


if __name__ == "__main__":
    main()
