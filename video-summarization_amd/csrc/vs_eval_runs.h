// vs_eval_runs.h - run-length compression and ranks of a frame vector, shared by the host evaluation (vs_eval.cpp) and
// the host side of the device evaluation (vs_eval_device.cpp).  Internal: not part of the C ABI.
#pragma once
#include <algorithm>
#include <numeric>
#include <vector>

namespace vs_eval_detail {

// ---- rank correlations on RUN-LENGTH-COMPRESSED frame vectors ----
// Both inputs of evaluate_scores are piecewise constant: the prediction is up-sampled from one score per pick (15 frames,
// compute_metrics.py:30-37) and the users' importance scores are per-shot integers (TVSum: 1..5 over 2-second shots).  A
// frame vector is therefore held as runs (start, value), ranks are taken over run VALUES with the run lengths as weights,
// and Kendall's pair counts / Spearman's sums become weighted sums over the joint runs of the two vectors.  Every pair
// count is an exact integer and every Spearman sum an exact multiple of 1/4 (far below 2^53), so the results are the
// ones of the per-frame computation (scipy.stats.rankdata(-x, 'average'), kendalltau variant 'b', np.corrcoef) bit for
// bit; vectors without runs cost what the per-frame form costs.
struct Ranked {
    int n = 0;                          // frames
    std::vector<int> start;             // run r covers frames [start[r], start[r+1]); start.back() == n
    std::vector<int> dense;             // per run: index of its value among the distinct values, largest value first (rank order)
    std::vector<long long> gweight;     // per distinct value: frames holding it
    std::vector<double> grank;          // per distinct value: the average rank of those frames
};

// per-thread work vectors: they keep their capacity from task to task (a fresh std::vector per task grows its thread's
// malloc arena by system calls, which serialise on the process' address-space lock: measured, no speed-up at all from
// 8 threads before this)
struct Scratch {
    std::vector<double> val;
    std::vector<int> order, cnt, cx;
    std::vector<long long> bit;
    struct Seg { long long w; int x, y; };
    std::vector<Seg> seg, tmp;
};

template <class T>
void rank_runs(const T *x, int n, Ranked &R, Scratch &W) {
    R.n = n;
    R.start.clear();
    std::vector<double> &val = W.val;
    val.clear();
    for (int i = 0; i < n; ++i)
        if (i == 0 || !((double)x[i] == (double)x[i - 1])) { R.start.push_back(i); val.push_back((double)x[i]); }
    const int m = (int)val.size();
    R.start.push_back(n);
    std::vector<int> &order = W.order;
    order.resize(m);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return val[a] > val[b]; });      // rankdata(-x): largest first
    R.dense.assign(m, 0);
    R.gweight.clear();
    for (int k = 0; k < m; ++k) {
        const int r = order[k];
        if (k == 0 || !(val[r] == val[order[k - 1]])) R.gweight.push_back(0);
        R.dense[r] = (int)R.gweight.size() - 1;
        R.gweight.back() += R.start[r + 1] - R.start[r];
    }
    R.grank.resize(R.gweight.size());
    long long before = 0;
    for (size_t g = 0; g < R.gweight.size(); ++g) {
        R.grank[g] = (double)before + 0.5 * (double)(R.gweight[g] + 1);          // average of before+1 .. before+c
        before += R.gweight[g];
    }
}

}  // namespace vs_eval_detail
