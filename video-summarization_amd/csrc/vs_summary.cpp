// vs_summary.cpp — host side of the keyshot summary on the device (include/vs_summary.h): the argument checks, the small
// per-call tables (one entry per pick segment and per shot - never per frame), the workspace layout, the three launches
// and the one download of the per-video counts, the selection and the shot means.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vs_error.h"
#include "vs_eval_device_kernels.h"
#include "vs_scorer.h"
#include "vs_summary.h"
#include "vs_summary_kernels.h"

namespace {

constexpr int32_t kMaxFrames = 1 << 18;          // the shot mean's pairwise walk (vs_keyshot_device.h) is sized for it
constexpr int32_t kMaxSummary = 1 << 24;         // frames of one summary
constexpr int32_t kMaxVideos = 65535;            // summary_fill's grid has the video in its second dimension

int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// the tables as they are staged on the host, and where everything lies in the workspace
struct Plan {
    std::vector<SmVideo> vid;
    std::vector<SmSeg> seg;
    std::vector<int32_t> shot_lo, shot_hi, shot_wt, shot_clip, ne_start, ne_end, ne_shot;
    int64_t n_shots = 0, n_frames = 0, n_out = 0, seg_cap = 0;
    int32_t max_L = 0;
    // the upload (one copy), the download (one copy), then what stays on the device
    int64_t o_vid = 0, o_seg = 0, o_lo = 0, o_hi = 0, o_wt = 0, o_clip = 0, o_ns = 0, o_ne = 0, o_nshot = 0, up_end = 0;
    int64_t o_vidout = 0, o_val = 0, o_sel = 0, down_end = 0;
    int64_t o_src = 0, o_dst = 0, o_bits = 0, o_rows = 0, total = 0;
};

// Checks everything that needs no GPU and lays the call out.  positions == NULL (the workspace query): the pick
// segments are not built, only counted by their upper bound n_positions + 1 per video - the layout is the same.
int make_plan(int32_t n_videos, const int32_t *n_scores, const int32_t *n_positions, const int32_t *n_frames, const int32_t *n_shots,
              const int32_t *positions, const int32_t *change_points, double proportion, Plan &P) {
    if (n_videos < 1 || n_videos > kMaxVideos) return vs_failf(VS_ERR_INVALID, "summarize: n_videos=%d outside [1, %d]", n_videos, kMaxVideos);
    if (!n_positions || !n_frames || !n_shots || !change_points)
        return vs_failf(VS_ERR_INVALID, "summarize: n_positions / n_frames / n_shots / change_points is NULL");
    if (!(proportion >= 0.0 && proportion <= 1.0))             // also false for a NaN
        return vs_failf(VS_ERR_INVALID, "summarize: proportion=%g is not in [0, 1]", proportion);
    P.vid.resize(n_videos);
    int64_t pos_at = 0, score_at = 0, bits = 0, rows = 0;
    for (int32_t v = 0; v < n_videos; ++v) {
        const int32_t nf = n_frames[v], ns = n_shots[v], np0 = n_positions[v], nsc = n_scores ? n_scores[v] : 0;
        if (ns < 1 || np0 < 1 || nf < 0 || nsc < 0)
            return vs_failf(VS_ERR_INVALID, "summarize: video %d has an empty or negative field (n_shots=%d n_positions=%d n_frames=%d n_scores=%d)",
                        v, ns, np0, nf, nsc);
        if (nf > kMaxFrames) return vs_failf(VS_ERR_INVALID, "summarize: video %d: n_frames=%d above %d", v, nf, kMaxFrames);
        SmVideo &E = P.vid[v];
        E = SmVideo{};
        E.n_frames = nf; E.n_shots = ns;
        E.score_off = score_at; E.frame_off = P.n_frames; E.shot_off = P.n_shots; E.ne_off = (int64_t)P.ne_start.size();
        E.out_off = P.n_out;

        // pick segments: upsample() of vs_eval.cpp with the pick's index in place of its score
        if (positions) {
            const int32_t *pos = positions + pos_at;
            for (int i = 1; i < np0; ++i)
                if (pos[i] < pos[i - 1])
                    return vs_failf(VS_ERR_INVALID, "summarize: video %d: positions decrease at %d (%d after %d)", v, i, pos[i], pos[i - 1]);
            const int np_ = np0 + (pos[np0 - 1] != nf ? 1 : 0);
            auto at = [&](int i) { return std::max(0, std::min(i < np0 ? pos[i] : nf, nf)); };
            if (np_ - 1 > nsc + 1)
                return vs_failf(VS_ERR_INVALID, "summarize: video %d: more pick segments (%d) than scores + 1 (%d)", v, np_ - 1, nsc + 1);
            const int first = np_ > 1 ? at(0) : nf;             // frames before the first segment hold 0
            if (first > 0) P.seg.push_back(SmSeg{E.frame_off, 0, first, -1, 0});
            for (int i = 0; i + 1 < np_; ++i) {
                const int lo = at(i), hi = at(i + 1);
                if (hi > lo) P.seg.push_back(SmSeg{E.frame_off, lo, hi, i == nsc ? -1 : i, 0});
            }
        }
        P.seg_cap += (int64_t)np0 + 1;

        // shots: generate_summary.py:41-46 and the summary's frames
        const int32_t *cp = change_points + 2 * P.n_shots;
        const int32_t last_end = cp[2 * (ns - 1) + 1];
        if (last_end < 0) return vs_failf(VS_ERR_INVALID, "summarize: video %d: the last shot ends before frame 0", v);
        if (last_end >= kMaxSummary) return vs_failf(VS_ERR_INVALID, "summarize: video %d: the last shot ends at %d, above %d", v, last_end, kMaxSummary - 1);
        E.L = last_end + 1;
        E.W = (int)((double)(last_end + 1) * proportion);
        int prev_end = -1;
        for (int s = 0; s < ns; ++s) {
            const int32_t a = cp[2 * s], b = cp[2 * s + 1];
            const int64_t wt = (int64_t)b - a + 1;
            if (wt < 0) return vs_failf(VS_ERR_INVALID, "summarize: video %d: shot %d has a negative length", v, s);
            if (wt > INT32_MAX) return vs_failf(VS_ERR_INVALID, "summarize: video %d: shot %d is longer than 2^31 - 1 frames", v, s);
            const int lo = std::max(0, std::min(a, nf)), hi = std::max(lo, (int)std::min<int64_t>((int64_t)b + 1, nf));
            P.shot_lo.push_back(lo); P.shot_hi.push_back(hi); P.shot_wt.push_back((int32_t)wt);
            const int ca = std::max(0, a), cb = std::min(last_end, b);
            const int clip = std::max(0, cb - ca + 1);
            if (clip > 0) {
                if (ca <= prev_end) return vs_failf(VS_ERR_INVALID, "summarize: video %d: shot %d overlaps or precedes an earlier shot", v, s);
                prev_end = cb;
                P.ne_start.push_back(ca); P.ne_end.push_back(cb); P.ne_shot.push_back(s);
            }
            P.shot_clip.push_back(clip);
        }
        E.n_ne = (int32_t)((int64_t)P.ne_start.size() - E.ne_off);
        E.bits_off = bits; bits += (int64_t)ns * ((E.W + 64) / 64);
        if (E.W + 1 > EV_LDS_COLS) { E.rows_off = rows; rows += 2 * ((int64_t)E.W + 1); }
        else E.rows_off = -1;
        P.max_L = std::max(P.max_L, E.L);
        pos_at += np0; score_at += nsc;
        P.n_shots += ns; P.n_frames += nf; P.n_out += E.L;
    }
    int64_t off = 0;
    auto take = [&](int64_t bytes) { const int64_t at = off; off = align256(off + bytes); return at; };
    P.o_vid = take((int64_t)n_videos * (int64_t)sizeof(SmVideo));
    P.o_seg = take(P.seg_cap * (int64_t)sizeof(SmSeg));
    P.o_lo = take(P.n_shots * 4); P.o_hi = take(P.n_shots * 4); P.o_wt = take(P.n_shots * 4); P.o_clip = take(P.n_shots * 4);
    P.o_ns = take(P.n_shots * 4); P.o_ne = take(P.n_shots * 4); P.o_nshot = take(P.n_shots * 4);
    P.up_end = off;
    P.o_vidout = off; off += (int64_t)n_videos * 2 * 8;              // the download: 8-byte fields, then 1-byte
    P.o_val = off; off += P.n_shots * 8;
    P.o_sel = off; off += P.n_shots;
    P.down_end = off; off = align256(off);
    P.o_src = take(P.n_frames * 4);
    P.o_dst = take(P.n_shots * 4);
    P.o_bits = take(bits * 8);
    P.o_rows = take(rows * 8);
    P.total = off;
    return VS_OK;
}

}  // namespace

extern "C" {

size_t vs_summarize_workspace_bytes(int32_t n_videos, const int32_t *n_positions, const int32_t *n_frames, const int32_t *n_shots,
                                    const int32_t *change_points, double proportion) {
    Plan P;
    if (make_plan(n_videos, nullptr, n_positions, n_frames, n_shots, nullptr, change_points, proportion, P) != VS_OK) return 0;
    return (size_t)P.total;
}

int vs_summarize(int32_t n_videos, const int32_t *n_scores, const int32_t *n_positions, const int32_t *n_frames, const int32_t *n_shots,
                 const int32_t *positions, const int32_t *change_points, double proportion, const float *scores_dev,
                 int8_t *summary_dev, int32_t *frames_dev, int32_t *n_selected_frames, int8_t *selected_shots_or_null,
                 double *shot_means_or_null, void *workspace, size_t workspace_bytes, void *stream) {
    if (!n_scores || !positions) return vs_failf(VS_ERR_INVALID, "summarize: n_scores / positions is NULL");
    Plan P;
    if (int rc = make_plan(n_videos, n_scores, n_positions, n_frames, n_shots, positions, change_points, proportion, P)) return rc;
    if (!scores_dev || !summary_dev || !frames_dev || !n_selected_frames)
        return vs_failf(VS_ERR_INVALID, "summarize: scores_dev / summary_dev / frames_dev / n_selected_frames is NULL");
    if (!workspace) return vs_failf(VS_ERR_INVALID, "summarize: workspace is NULL");
    if (workspace_bytes < (size_t)P.total)
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %lld needed", workspace_bytes, (long long)P.total);
    if (((uintptr_t)workspace & 255) != 0) return vs_failf(VS_ERR_INVALID, "summarize: workspace is not 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;

    std::vector<char> up((size_t)P.up_end, 0);
    auto put = [&](int64_t at, const void *src, size_t bytes) { if (bytes) std::memcpy(up.data() + at, src, bytes); };
    put(P.o_vid, P.vid.data(), P.vid.size() * sizeof(SmVideo));
    put(P.o_seg, P.seg.data(), P.seg.size() * sizeof(SmSeg));
    put(P.o_lo, P.shot_lo.data(), P.shot_lo.size() * 4); put(P.o_hi, P.shot_hi.data(), P.shot_hi.size() * 4);
    put(P.o_wt, P.shot_wt.data(), P.shot_wt.size() * 4); put(P.o_clip, P.shot_clip.data(), P.shot_clip.size() * 4);
    put(P.o_ns, P.ne_start.data(), P.ne_start.size() * 4); put(P.o_ne, P.ne_end.data(), P.ne_end.size() * 4);
    put(P.o_nshot, P.ne_shot.data(), P.ne_shot.size() * 4);
    VS_HIP(hipMemcpyAsync(ws, up.data(), up.size(), hipMemcpyHostToDevice, st));

    SmArgs A{};
    A.vid = (const SmVideo *)(ws + P.o_vid); A.seg = (const SmSeg *)(ws + P.o_seg); A.n_seg = (int64_t)P.seg.size();
    A.shot_lo = (const int32_t *)(ws + P.o_lo); A.shot_hi = (const int32_t *)(ws + P.o_hi); A.shot_wt = (const int32_t *)(ws + P.o_wt);
    A.shot_clip = (const int32_t *)(ws + P.o_clip); A.ne_start = (const int32_t *)(ws + P.o_ns); A.ne_end = (const int32_t *)(ws + P.o_ne);
    A.ne_shot = (const int32_t *)(ws + P.o_nshot); A.scores = scores_dev;
    A.frame_src = (int32_t *)(ws + P.o_src); A.shot_dst = (int32_t *)(ws + P.o_dst); A.vidout = (int64_t *)(ws + P.o_vidout);
    A.val = (double *)(ws + P.o_val); A.sel = (int8_t *)(ws + P.o_sel); A.bits = (unsigned long long *)(ws + P.o_bits);
    A.rows = (double *)(ws + P.o_rows); A.summary = summary_dev; A.frames = frames_dev;
    VS_LAUNCH_HIP(vsk_summary_expand_picks(A, st));
    VS_LAUNCH_HIP(vsk_summary_select(A, n_videos, st));
    VS_LAUNCH_HIP(vsk_summary_fill(A, n_videos, P.max_L, st));
    std::vector<char> down((size_t)(P.down_end - P.o_vidout));
    VS_HIP(hipMemcpyAsync(down.data(), ws + P.o_vidout, down.size(), hipMemcpyDeviceToHost, st));
    VS_HIP(hipStreamSynchronize(st));

    const int64_t *vidout = (const int64_t *)down.data();
    for (int32_t v = 0; v < n_videos; ++v)
        if (vidout[2 * (size_t)v + 1] != 0)
            return vs_failf(VS_ERR_INVALID, "summarize: video %d: capacity index out of range in the knapsack back-track (IndexError in the reference)", v);
    for (int32_t v = 0; v < n_videos; ++v) n_selected_frames[v] = (int32_t)vidout[2 * (size_t)v];
    if (shot_means_or_null) std::memcpy(shot_means_or_null, down.data() + (P.o_val - P.o_vidout), (size_t)P.n_shots * 8);
    if (selected_shots_or_null) std::memcpy(selected_shots_or_null, down.data() + (P.o_sel - P.o_vidout), (size_t)P.n_shots);
    return VS_OK;
}

}  // extern "C"
