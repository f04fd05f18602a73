// vs_eval_device.cpp — host side of the keyshot evaluation on the device (include/vs_eval_device.h): the static part of a
// set (everything that does not depend on the scores, built once with the host evaluation's own run and rank code), the
// per-run plan and workspace layout, the launches, and the last double operations per (video, user) - the very
// expressions of vs_eval.cpp, on the exact integers the kernels return.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "vs_error.h"
#include "vs_eval_device.h"
#include "vs_eval_device_kernels.h"
#include "vs_eval_runs.h"
#include "vs_scorer.h"

namespace {

using vs_eval_detail::Ranked;
using vs_eval_detail::Scratch;
using vs_eval_detail::rank_runs;

// 4 * saa, 4 * sbb and 4 * sab are at most n^3 / 3 (the untied case): exact in int64 and, divided by 4, in double
constexpr int32_t kMaxFrames = 1 << 18;

int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// the flat static arrays as they are built on the host
struct Flat {
    std::vector<EvVideo> vid;
    std::vector<EvPair> pairs;
    std::vector<int32_t> frame_src, shot_lo, shot_hi, shot_wt, shot_clip, cnt, xrun_src, xrun_w, jw, jx, jy;
};

struct Plan {
    std::vector<int32_t> ids;
    std::vector<char> up;                        // slots, then tasks: one upload
    int32_t n_tasks = 0, n_pairs = 0;
    int64_t n_users = 0, n_shots = 0, n_xruns = 0;
    int64_t tasks_off = 0, vidout_off = 0, pairout_off = 0, ov_off = 0, sel_off = 0, down_end = 0;
    int64_t val_off = 0, rank_off = 0, bits_off = 0, rows_off = 0, total = 0;
};

}  // namespace

struct vs_eval_set {
    std::vector<EvVideo> vid;
    std::vector<EvPair> pairs;                   // host copy: the plan orders the tasks by their joint-run counts
    std::vector<int64_t> user_off;               // per video: its first entry of sumG
    std::vector<long long> sumG;                 // per (video, summary user)
    std::vector<long long> ytie, sbb4;           // per (video, score user), indexed like pairs
    std::vector<char> use_max, has_scores;
    Flat pending;                                // the static arrays until they are uploaded (uploaded == false)
    bool uploaded = false;
    void *dev = nullptr;                         // the one device allocation behind S
    EvStatic S{};
    Plan plan;                                   // of the last run: an epoch loop asks for the same videos every time
    std::vector<char> down;                      // host end of a run's one download
};

namespace {

int check_record(const vs_eval_video &V, int v) {
    if (!V.positions || !V.change_points || !V.user_summary)
        return vs_failf(VS_ERR_INVALID, "eval_set: video %d has a NULL positions / change_points / user_summary", v);
    if (V.n_shots < 1 || V.n_users < 1 || V.n_positions < 1 || V.n_frames < 0 || V.n_scores < 0 || V.user_len < 0)
        return vs_failf(VS_ERR_INVALID, "eval_set: video %d has an empty or negative field (n_shots=%d n_users=%d n_positions=%d n_frames=%d n_scores=%d)",
                    v, V.n_shots, V.n_users, V.n_positions, V.n_frames, V.n_scores);
    if (V.user_scores && (V.n_score_users < 1 || V.n_frames < 2))
        return vs_failf(VS_ERR_INVALID, "eval_set: video %d: user_scores needs n_score_users >= 1 and n_frames >= 2", v);
    if (V.n_frames > kMaxFrames) return vs_failf(VS_ERR_INVALID, "eval_set: video %d: n_frames=%d above %d", v, V.n_frames, kMaxFrames);
    return VS_OK;
}

// the static part of one video, appended to F and to the set's host tables
int build_video(const vs_eval_video &V, int v, Flat &F, vs_eval_set &set, Ranked &Y, Scratch &scratch) {
    EvVideo E{};
    const int nf = V.n_frames;
    E.n_frames = nf; E.n_shots = V.n_shots; E.n_users = V.n_users; E.n_scores = V.n_scores;
    E.n_score_users = V.user_scores ? V.n_score_users : 0;
    E.frame_off = (int64_t)F.frame_src.size();
    E.shot_off = (int64_t)F.shot_lo.size();
    E.cnt_off = (int64_t)F.cnt.size();
    E.xrun_off = (int64_t)F.xrun_src.size();
    E.pair_off = (int64_t)F.pairs.size();

    // upsample() of vs_eval.cpp with the pick's index in place of its score: -1 where the value is 0
    F.frame_src.resize(F.frame_src.size() + (size_t)nf, -1);
    int32_t *src = F.frame_src.data() + E.frame_off;
    const int np_ = V.n_positions + (V.positions[V.n_positions - 1] != nf ? 1 : 0);
    auto pos = [&](int i) { return i < V.n_positions ? V.positions[i] : nf; };
    for (int i = 0; i + 1 < np_; ++i) {
        const int lo = std::max(0, std::min(pos(i), nf)), hi = std::max(0, std::min(pos(i + 1), nf));
        if (i > V.n_scores) return vs_failf(VS_ERR_INVALID, "eval_set: video %d: more pick segments than scores + 1", v);
        for (int f = lo; f < hi; ++f) src[f] = i == V.n_scores ? -1 : i;
    }
    std::vector<int> xstart;                      // run r of the prediction covers frames [xstart[r], xstart[r + 1])
    for (int f = 0; f < nf; ++f)
        if (f == 0 || src[f] != src[f - 1]) { xstart.push_back(f); F.xrun_src.push_back(src[f]); }
    xstart.push_back(nf);
    E.n_xruns = (int32_t)xstart.size() - 1;
    for (int r = 0; r < E.n_xruns; ++r) F.xrun_w.push_back(xstart[r + 1] - xstart[r]);

    // shots: generate_summary.py:41-46 and the summary's frames
    const int last_end = V.change_points[2 * (V.n_shots - 1) + 1];
    if (last_end < 0) return vs_failf(VS_ERR_INVALID, "eval_set: video %d: the last shot ends before frame 0", v);
    const int summary_len = last_end + 1;
    E.W = (int)((double)(last_end + 1) * 0.15);
    std::vector<int> ca(V.n_shots), cb(V.n_shots);
    int prev_end = -1;
    for (int s = 0; s < V.n_shots; ++s) {
        const int a = V.change_points[2 * s], b = V.change_points[2 * s + 1];
        if (b - a + 1 < 0) return vs_failf(VS_ERR_INVALID, "eval_set: video %d: shot %d has a negative length", v, s);
        const int lo = std::max(0, std::min(a, nf)), hi = std::max(lo, std::min(b + 1, nf));
        F.shot_lo.push_back(lo); F.shot_hi.push_back(hi); F.shot_wt.push_back(b - a + 1);
        ca[s] = std::max(0, a); cb[s] = std::min(summary_len - 1, b);
        const int clip = std::max(0, cb[s] - ca[s] + 1);
        if (clip > 0) {
            if (ca[s] <= prev_end) return vs_failf(VS_ERR_INVALID, "eval_set: video %d: shot %d overlaps or precedes an earlier shot", v, s);
            prev_end = cb[s];
        }
        F.shot_clip.push_back(clip);
    }

    // the users' summaries, counted per shot (evaluation_metrics.py:12-24: the overlap runs over the common length)
    set.user_off.push_back((int64_t)set.sumG.size());
    const int common = std::min(summary_len, V.user_len);
    std::vector<int32_t> prefix((size_t)V.user_len + 1);
    for (int u = 0; u < V.n_users; ++u) {
        const int8_t *g = V.user_summary + (size_t)u * V.user_len;
        prefix[0] = 0;
        for (int i = 0; i < V.user_len; ++i) prefix[i + 1] = prefix[i] + g[i];
        set.sumG.push_back(prefix[V.user_len]);
        for (int s = 0; s < V.n_shots; ++s) {
            const int lo = std::min(ca[s], common), hi = std::max(lo, std::min(cb[s] + 1, common));
            F.cnt.push_back(prefix[hi] - prefix[lo]);
        }
    }

    // the users' importance scores: runs, dense rank groups, doubled average ranks, ytie, 4 sbb, joint runs
    for (int u = 0; u < E.n_score_users; ++u) {
        if (V.user_scores_f32) rank_runs((const float *)V.user_scores + (size_t)u * nf, nf, Y, scratch);
        else rank_runs((const double *)V.user_scores + (size_t)u * nf, nf, Y, scratch);
        std::vector<int32_t> r2y(Y.gweight.size());
        long long before = 0, ytie = 0, sbb4 = 0;
        for (size_t g = 0; g < Y.gweight.size(); ++g) {
            const long long c = Y.gweight[g];
            r2y[g] = (int32_t)(2 * before + c + 1);
            const long long d = (long long)r2y[g] - (nf + 1);
            ytie += c * (c - 1) / 2;
            sbb4 += c * d * d;
            before += c;
        }
        EvPair P{};
        P.j_off = (int64_t)F.jw.size();
        const size_t ny = Y.dense.size();
        for (size_t rx = 0, ry = 0; rx < (size_t)E.n_xruns && ry < ny;) {
            const int lo = std::max(xstart[rx], Y.start[ry]), hi = std::min(xstart[rx + 1], Y.start[ry + 1]);
            if (hi > lo) { F.jw.push_back(hi - lo); F.jx.push_back((int32_t)rx); F.jy.push_back(r2y[Y.dense[ry]]); }
            if (xstart[rx + 1] <= Y.start[ry + 1]) ++rx; else ++ry;
        }
        P.m = (int32_t)((int64_t)F.jw.size() - P.j_off);
        F.pairs.push_back(P);
        set.ytie.push_back(ytie);
        set.sbb4.push_back(sbb4);
    }
    F.vid.push_back(E);
    set.use_max.push_back(V.use_max != 0);
    set.has_scores.push_back(V.user_scores != nullptr);
    return VS_OK;
}

template <class T>
int64_t place(int64_t &off, const std::vector<T> &v) {
    const int64_t at = off;
    off = align256(off + (int64_t)(v.size() * sizeof(T)));
    return at;
}

// The static arrays go to the device ONCE: at creation where a device is present, else (a set created on a host without
// one, as the argument checks' tests do) by the first run.
int upload(vs_eval_set &set, hipStream_t st) {
    if (set.uploaded) return VS_OK;
    const Flat &F = set.pending;
    int64_t off = 0;
    const int64_t o_vid = place(off, F.vid), o_pairs = place(off, F.pairs), o_src = place(off, F.frame_src),
                  o_lo = place(off, F.shot_lo), o_hi = place(off, F.shot_hi), o_wt = place(off, F.shot_wt),
                  o_clip = place(off, F.shot_clip), o_cnt = place(off, F.cnt), o_xs = place(off, F.xrun_src),
                  o_xw = place(off, F.xrun_w), o_jw = place(off, F.jw), o_jx = place(off, F.jx), o_jy = place(off, F.jy);
    VS_HIP(hipMalloc(&set.dev, (size_t)std::max<int64_t>(off, 256)));
    char *d = (char *)set.dev;
#define EV_PUT(o, v) \
    if (!(v).empty()) VS_HIP(hipMemcpyAsync(d + (o), (v).data(), (v).size() * sizeof((v)[0]), hipMemcpyHostToDevice, st))
    EV_PUT(o_vid, F.vid); EV_PUT(o_pairs, F.pairs); EV_PUT(o_src, F.frame_src); EV_PUT(o_lo, F.shot_lo); EV_PUT(o_hi, F.shot_hi);
    EV_PUT(o_wt, F.shot_wt); EV_PUT(o_clip, F.shot_clip); EV_PUT(o_cnt, F.cnt); EV_PUT(o_xs, F.xrun_src); EV_PUT(o_xw, F.xrun_w);
    EV_PUT(o_jw, F.jw); EV_PUT(o_jx, F.jx); EV_PUT(o_jy, F.jy);
#undef EV_PUT
    VS_HIP(hipStreamSynchronize(st));
    EvStatic &S = set.S;
    S.vid = (const EvVideo *)(d + o_vid); S.pairs = (const EvPair *)(d + o_pairs); S.frame_src = (const int32_t *)(d + o_src);
    S.shot_lo = (const int32_t *)(d + o_lo); S.shot_hi = (const int32_t *)(d + o_hi); S.shot_wt = (const int32_t *)(d + o_wt);
    S.shot_clip = (const int32_t *)(d + o_clip); S.cnt = (const int32_t *)(d + o_cnt); S.xrun_src = (const int32_t *)(d + o_xs);
    S.xrun_w = (const int32_t *)(d + o_xw); S.jw = (const int32_t *)(d + o_jw); S.jx = (const int32_t *)(d + o_jx);
    S.jy = (const int32_t *)(d + o_jy);
    set.uploaded = true;
    set.pending = Flat{};
    return VS_OK;
}

// Checks the ids (no GPU) and lays out the run: slots in video_ids order, (slot, user) tasks with the most joint runs first
// (the long pairs should not start last), the workspace.  The last plan is kept: same ids, nothing to do.
int make_plan(const vs_eval_set *set, const int32_t *ids, int32_t n_ids, Plan &P) {
    if (!set) return vs_failf(VS_ERR_INVALID, "eval_set: set is NULL");
    if (!ids || n_ids < 1) return vs_failf(VS_ERR_INVALID, "eval_set: video_ids is NULL or empty");
    const int32_t nv = (int32_t)set->vid.size();
    for (int32_t i = 0; i < n_ids; ++i)
        if (ids[i] < 0 || ids[i] >= nv) return vs_failf(VS_ERR_INVALID, "eval_set: video_ids[%d]=%d outside [0, %d)", i, ids[i], nv);
    if ((int32_t)P.ids.size() == n_ids && std::equal(ids, ids + n_ids, P.ids.begin())) return VS_OK;
    P = Plan{};
    P.ids.assign(ids, ids + n_ids);
    std::vector<EvSlot> slots(n_ids);
    std::vector<EvTask> tasks;
    std::vector<int32_t> weight;
    int64_t scores = 0, bits = 0, rows = 0;
    for (int32_t i = 0; i < n_ids; ++i) {
        const EvVideo &V = set->vid[ids[i]];
        EvSlot &s = slots[i];
        s.video = ids[i];
        s.score_off = (int32_t)scores; scores += V.n_scores;
        s.shot_out = (int32_t)P.n_shots; P.n_shots += V.n_shots;
        s.user_out = (int32_t)P.n_users; P.n_users += V.n_users;
        s.xrun_out = (int32_t)P.n_xruns; P.n_xruns += V.n_xruns;
        s.pair_out = P.n_pairs; P.n_pairs += V.n_score_users;
        s.bits_off = bits; bits += (int64_t)V.n_shots * ((V.W + 64) / 64);
        if (V.W + 1 > EV_LDS_COLS) { s.rows_off = rows; rows += 2 * ((int64_t)V.W + 1); }
        else s.rows_off = -1;
        for (int32_t u = 0; u < V.n_score_users; ++u) { tasks.push_back(EvTask{i, u}); weight.push_back(set->pairs[V.pair_off + u].m); }
        if (scores > INT32_MAX || P.n_shots > INT32_MAX || P.n_users > INT32_MAX || P.n_xruns > INT32_MAX)
            return vs_failf(VS_ERR_INVALID, "eval_set: the listed videos exceed 2^31 scores, shots, users or runs");
    }
    std::vector<int32_t> order(tasks.size());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return weight[a] > weight[b]; });
    P.n_tasks = (int32_t)tasks.size();
    int64_t off = 0;
    off = align256((int64_t)n_ids * (int64_t)sizeof(EvSlot));
    P.tasks_off = off; off = align256(off + (int64_t)tasks.size() * (int64_t)sizeof(EvTask));
    P.up.assign((size_t)off, 0);
    std::memcpy(P.up.data(), slots.data(), slots.size() * sizeof(EvSlot));
    for (size_t k = 0; k < order.size(); ++k) std::memcpy(P.up.data() + P.tasks_off + k * sizeof(EvTask), &tasks[order[k]], sizeof(EvTask));
    P.vidout_off = off; off += (int64_t)n_ids * 4 * 8;                // the download: 8-byte, then 4-byte, then 1-byte fields
    P.pairout_off = off; off += (int64_t)P.n_pairs * 3 * 8;
    P.ov_off = off; off += P.n_users * 4;
    P.sel_off = off; off += P.n_shots;
    P.down_end = off; off = align256(off);
    P.val_off = off; off = align256(off + P.n_shots * 8);
    P.rank_off = off; off = align256(off + P.n_xruns * 4);
    P.bits_off = off; off = align256(off + bits * 8);
    P.rows_off = off; off = align256(off + rows * 8);
    P.total = off;
    return VS_OK;
}

}  // namespace

extern "C" {

int vs_eval_set_create(const vs_eval_video *videos, int32_t n_videos, void *stream, vs_eval_set **out) {
    if (!out) return vs_failf(VS_ERR_INVALID, "eval_set: out is NULL");
    *out = nullptr;
    if (!videos || n_videos < 1) return vs_failf(VS_ERR_INVALID, "eval_set: videos is NULL or n_videos < 1");
    for (int32_t v = 0; v < n_videos; ++v)
        if (int rc = check_record(videos[v], v)) return rc;
    vs_eval_set *set = new vs_eval_set;
    Flat &F = set->pending;
    Ranked Y;
    Scratch scratch;
    int rc = VS_OK;
    for (int32_t v = 0; v < n_videos && rc == VS_OK; ++v) rc = build_video(videos[v], v, F, *set, Y, scratch);
    if (rc == VS_OK) {
        set->vid = F.vid;
        set->pairs = F.pairs;
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) rc = upload(*set, (hipStream_t)stream);
    }
    if (rc != VS_OK) { vs_eval_set_free(set); return rc; }
    *out = set;
    return VS_OK;
}

void vs_eval_set_free(vs_eval_set *set) {
    if (!set) return;
    if (set->dev) (void)hipFree(set->dev);
    delete set;
}

size_t vs_eval_set_workspace_bytes(const vs_eval_set *set, const int32_t *video_ids, int32_t n_ids) {
    Plan P;
    if (make_plan(set, video_ids, n_ids, P) != VS_OK) return 0;
    return (size_t)P.total;
}

int vs_eval_set_run(vs_eval_set *set, const float *scores_dev, const int32_t *video_ids, int32_t n_ids, double *f_score,
                    double *kendall, double *spearman, int8_t *selected_or_null, void *workspace, size_t workspace_bytes,
                    void *stream) {
    if (!set) return vs_failf(VS_ERR_INVALID, "eval_set: set is NULL");
    Plan &P = set->plan;
    if (int rc = make_plan(set, video_ids, n_ids, P)) { P = Plan{}; return rc; }
    if (!scores_dev || !f_score || !kendall || !spearman) return vs_failf(VS_ERR_INVALID, "eval_set: scores_dev / f_score / kendall / spearman is NULL");
    if (!workspace || workspace_bytes < (size_t)P.total)
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %lld needed", workspace_bytes, (long long)P.total);
    if (((uintptr_t)workspace & 255) != 0) return vs_failf(VS_ERR_INVALID, "eval_set: workspace is not 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    if (int rc = upload(*set, st)) return rc;
    VS_HIP(hipMemcpyAsync(ws, P.up.data(), P.up.size(), hipMemcpyHostToDevice, st));
    EvRun R{};
    R.slots = (const EvSlot *)ws; R.tasks = (const EvTask *)(ws + P.tasks_off); R.scores = scores_dev;
    R.vidout = (int64_t *)(ws + P.vidout_off); R.pairout = (int64_t *)(ws + P.pairout_off); R.ov = (int32_t *)(ws + P.ov_off);
    R.sel = (int8_t *)(ws + P.sel_off); R.val = (double *)(ws + P.val_off); R.rank2x = (int32_t *)(ws + P.rank_off);
    R.bits = (unsigned long long *)(ws + P.bits_off); R.rows = (double *)(ws + P.rows_off);
    VS_LAUNCH_HIP(vsk_eval_summary(set->S, R, n_ids, st));
    VS_LAUNCH_HIP(vsk_eval_xrank(set->S, R, n_ids, st));
    VS_LAUNCH_HIP(vsk_eval_pairs(set->S, R, P.n_tasks, st));
    set->down.resize((size_t)(P.down_end - P.vidout_off));
    VS_HIP(hipMemcpyAsync(set->down.data(), ws + P.vidout_off, set->down.size(), hipMemcpyDeviceToHost, st));
    VS_HIP(hipStreamSynchronize(st));

    const char *dn = set->down.data();
    const int64_t *vidout = (const int64_t *)dn, *pairout = (const int64_t *)(dn + (P.pairout_off - P.vidout_off));
    const int32_t *ov = (const int32_t *)(dn + (P.ov_off - P.vidout_off));
    const int8_t *sel = (const int8_t *)(dn + (P.sel_off - P.vidout_off));
    const EvSlot *slots = (const EvSlot *)P.up.data();
    for (int32_t i = 0; i < n_ids; ++i)
        if (vidout[4 * (size_t)i + 1] != 0)
            return vs_failf(VS_ERR_INVALID, "eval_set: video_ids[%d]=%d: capacity index out of range in the knapsack back-track (IndexError in the reference)",
                        i, video_ids[i]);
    if (selected_or_null) std::memcpy(selected_or_null, sel, (size_t)P.n_shots);
    auto pairs = [](long long c) { return c * (c - 1) / 2; };
    for (int32_t i = 0; i < n_ids; ++i) {
        const int v = video_ids[i];
        const EvVideo &V = set->vid[v];
        const EvSlot &sl = slots[i];
        // evaluate_summary, the expressions of vs_eval_fscore
        const long long sumS = vidout[4 * (size_t)i];
        double acc = 0.0, best = -INFINITY;
        for (int u = 0; u < V.n_users; ++u) {
            const long long o = ov[sl.user_out + u], sumG = set->sumG[set->user_off[v] + u];
            const double precision = (double)o / (double)sumS, recall = (double)o / (double)sumG;
            const double f = (precision + recall == 0) ? 0.0 : 2 * precision * recall * 100 / (precision + recall);
            acc += f;
            best = std::max(best, f);
        }
        f_score[i] = set->use_max[v] ? best : acc / V.n_users;
        if (!set->has_scores[v]) { kendall[i] = NAN; spearman[i] = NAN; continue; }
        // evaluate_scores, the expressions of vs_eval.cpp's correlate()
        const long long tot = pairs(V.n_frames), xtie = vidout[4 * (size_t)i + 2] / 2;
        const double saa = 0.25 * (double)vidout[4 * (size_t)i + 3];
        double ks = 0, ss = 0;
        for (int u = 0; u < V.n_score_users; ++u) {
            const int64_t *po = pairout + 3 * ((size_t)sl.pair_out + u);
            const long long dis = po[0], ntie = po[1], ytie = set->ytie[V.pair_off + u];
            const double sab = 0.25 * (double)po[2], sbb = 0.25 * (double)set->sbb4[V.pair_off + u];
            double tau;
            if (xtie == tot || ytie == tot) tau = NAN;
            else {
                const double con_minus_dis = (double)(tot - xtie - ytie + ntie - 2 * dis);
                tau = std::min(1.0, std::max(-1.0, con_minus_dis / std::sqrt((double)(tot - xtie)) / std::sqrt((double)(tot - ytie))));
            }
            const double rho = sab / std::sqrt(saa * sbb);
            ks += tau; ss += rho;
        }
        kendall[i] = ks / V.n_score_users;
        spearman[i] = ss / V.n_score_users;
    }
    return VS_OK;
}

}  // extern "C"
