// C ABI of kernel temporal segmentation (include/vs_segment.h): argument checks, the workspace plan, the stage order,
// and the host end of the model selection (penalty and argmin in double, the reference's expression order).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vs_error.h"
#include "vs_kernels.h"
#include "vs_scorer.h"
#include "vs_segment.h"
#include "vs_segment_kernels.h"

namespace {

constexpr int32_t kMaxFrames = 1 << 16;          // (n + 1)^2 doubles of W stay addressable with 32-bit row indices
constexpr int32_t kDefaultLmax = 100000;         // the reference's cpd_nonlin default

int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }
int32_t round32(int32_t v) { return (v + 31) / 32 * 32; }

struct Plan {
    std::vector<KtsVideo> vids;
    int64_t vids_off = 0, bias_off = 0, xpad_off = 0, total = 0;
    int32_t n_max = 0, m_max = 0, d_pad = 0;
    // the one-launch Gram (the *_k entry points): its video table and the row norms, after everything else
    std::vector<KtsGramVideo> gvids;
    int64_t gvids_off = 0, nrm_off = 0;
    int32_t tiles = 0;
};

// Checks everything that needs no GPU and lays out the workspace.  Returns VS_OK or VS_ERR_INVALID (message set).
int make_plan(const int32_t *cu, int32_t batch, int32_t d, int32_t input, const int32_t *ncp, const int32_t *lmin,
              const int32_t *lmax, int32_t mode, Plan &P) {
    if (!cu || !ncp) return vs_failf(VS_ERR_INVALID, "cu / ncp is NULL");
    if (batch <= 0) return vs_failf(VS_ERR_INVALID, "batch=%d must be positive", batch);
    if (input != VS_KTS_FEATURES_F32 && input != VS_KTS_KERNEL_F32 && input != VS_KTS_KERNEL_F64)
        return vs_failf(VS_ERR_INVALID, "input=%d is not a VS_KTS_* input kind", input);
    if (mode != VS_KTS_SCORES && mode != VS_KTS_BACKTRACK && mode != VS_KTS_AUTO)
        return vs_failf(VS_ERR_INVALID, "mode=%d is not a VS_KTS_* mode", mode);
    const bool feats = input == VS_KTS_FEATURES_F32;
    if (feats && d <= 0) return vs_failf(VS_ERR_INVALID, "d=%d must be positive for features", d);
    if (cu[0] != 0) return vs_failf(VS_ERR_INVALID, "cu[0]=%d must be 0", cu[0]);
    P.vids.assign(batch, KtsVideo{});
    P.d_pad = feats ? round32(d) : 0;
    int64_t off = align256((int64_t)batch * (int64_t)sizeof(KtsVideo));
    int64_t k_in = 0;                                    // byte offset of each video's K in the caller's buffer
    const int64_t esz = input == VS_KTS_KERNEL_F64 ? 8 : 4;
    for (int32_t b = 0; b < batch; ++b) {
        const int32_t n = cu[b + 1] - cu[b];
        const int32_t m = ncp[b];
        const int32_t lo = lmin ? lmin[b] : 1, hi = lmax ? lmax[b] : kDefaultLmax;
        if (n <= 0 || n > kMaxFrames) return vs_failf(VS_ERR_INVALID, "video %d: n=%d frames outside [1, %d]", b, n, kMaxFrames);
        if (m < 0) return vs_failf(VS_ERR_INVALID, "video %d: ncp=%d must be >= 0", b, m);
        if (!(hi >= lo && lo >= 1)) return vs_failf(VS_ERR_INVALID, "video %d: needs lmax >= lmin >= 1 (lmin=%d lmax=%d)", b, lo, hi);
        if ((int64_t)n < (int64_t)(m + 1) * lo)
            return vs_failf(VS_ERR_INVALID, "video %d: needs n >= (ncp + 1) * lmin (n=%d ncp=%d lmin=%d)", b, n, m, lo);
        if ((int64_t)n > (int64_t)(m + 1) * hi)
            return vs_failf(VS_ERR_INVALID, "video %d: needs n <= (ncp + 1) * lmax (n=%d ncp=%d lmax=%d)", b, n, m, hi);
        KtsVideo &V = P.vids[b];
        V.n = n; V.m = m; V.lmin = lo; V.lmax = hi; V.mbest = m;
        const int64_t ld = n + 1;
        if (feats) {
            V.ldk = round32(n);
        } else {
            V.ldk = n;
            V.k_off = k_in;
            k_in += (int64_t)n * n * esz;
        }
        if (n > P.n_max) P.n_max = n;
        if (m > P.m_max) P.m_max = m;
        V.w_off = off; off = align256(off + ld * ld * 8);
        V.t_off = off; off = align256(off + (int64_t)((n + KTS_CHUNK - 1) / KTS_CHUNK) * ld * 8);
        V.k1_off = off; off = align256(off + ld * 8);
        V.i_off = off; off = align256(off + 2 * ld * 8);
        if (mode != VS_KTS_SCORES) { V.p_off = off; off = align256(off + (int64_t)(m + 1) * ld * 4); }
        else V.p_off = -1;
    }
    for (int32_t b = 0; b < batch; ++b) {            // scores and change points contiguous: one copy each to the host
        P.vids[b].s_off = off;
        off += (int64_t)(P.vids[b].m + 1) * 8;
    }
    off = align256(off);
    for (int32_t b = 0; b < batch; ++b) {
        P.vids[b].c_off = off;
        off += (int64_t)P.vids[b].m * 4;
    }
    off = align256(off + 4);
    if (feats) {                                     // Gram: zero bias, one padded copy of X (reused per video), K
        P.bias_off = off; off = align256(off + (int64_t)round32(P.n_max) * 4);
        P.xpad_off = off; off = align256(off + (int64_t)round32(P.n_max) * P.d_pad * 4);
        for (int32_t b = 0; b < batch; ++b) {
            P.vids[b].k_off = off;
            off = align256(off + (int64_t)P.vids[b].n * P.vids[b].ldk * 4);
        }
    }
    P.total = off;
    return VS_OK;
}

// the Gram K_b = X_b X_b^T of every video on the exact-fp32 GEMM: X_b copied into a zero-padded [round32(n)][round32(d)]
// buffer (zero rows / columns add nothing), C = Xpad[:n] Xpad^T with a zero bias, row stride round32(n)
int gram(const float *x, int32_t d, const int32_t *cu, const Plan &P, char *ws, hipStream_t st) {
    float *bias = (float *)(ws + P.bias_off), *xpad = (float *)(ws + P.xpad_off);
    VS_HIP(hipMemsetAsync(bias, 0, (size_t)round32(P.n_max) * 4, st));
    for (size_t b = 0; b < P.vids.size(); ++b) {
        const KtsVideo &V = P.vids[b];
        const int32_t npad = V.ldk;
        if (d != P.d_pad) VS_HIP(hipMemsetAsync(xpad, 0, (size_t)npad * P.d_pad * 4, st));
        else if (npad > V.n) VS_HIP(hipMemsetAsync(xpad + (size_t)V.n * P.d_pad, 0, (size_t)(npad - V.n) * P.d_pad * 4, st));
        VS_HIP(hipMemcpy2DAsync(xpad, (size_t)P.d_pad * 4, x + (size_t)cu[b] * d, (size_t)d * 4, (size_t)d * 4, V.n,
                                 hipMemcpyDeviceToDevice, st));
        VS_LAUNCH(vsk_linear(xpad, xpad, nullptr, bias, (float *)(ws + V.k_off), V.n, npad, P.d_pad, 0, nullptr, 1, 0, st));
    }
    return VS_OK;
}

int upload(const Plan &P, char *ws, hipStream_t st) {
    VS_HIP(hipMemcpyAsync(ws, P.vids.data(), P.vids.size() * sizeof(KtsVideo), hipMemcpyHostToDevice, st));
    return VS_OK;
}

// K (computed or the caller's) -> scatter table
int table(const void *x, int32_t input, int32_t d, const int32_t *cu, const Plan &P, char *ws, hipStream_t st) {
    const int B = (int)P.vids.size();
    if (int rc = upload(P, ws, st)) return rc;
    const KtsVideo *dv = (const KtsVideo *)ws;
    if (input == VS_KTS_FEATURES_F32) {
        if (int rc = gram((const float *)x, d, cu, P, ws, st)) return rc;
        VS_LAUNCH(vsk_kts_scatter_table(dv, B, P.n_max, ws, ws, 0, st));
    } else {
        VS_LAUNCH(vsk_kts_scatter_table(dv, B, P.n_max, ws, x, input == VS_KTS_KERNEL_F64, st));
    }
    return VS_OK;
}


int check_kernel(const vs_kts_kernel *kern) {
    if (!kern) return vs_failf(VS_ERR_INVALID, "kern is NULL");
    if (kern->kind != VS_KTS_GRAM_DOT && kern->kind != VS_KTS_GRAM_COSINE && kern->kind != VS_KTS_GRAM_RBF)
        return vs_failf(VS_ERR_INVALID, "kern->kind=%d is not a VS_KTS_GRAM_* kind", kern->kind);
    if (kern->reserved != 0) return vs_failf(VS_ERR_INVALID, "kern->reserved=%d must be 0", kern->reserved);
    if (kern->kind == VS_KTS_GRAM_RBF && !(std::isfinite(kern->gamma) && kern->gamma > 0.0))
        return vs_failf(VS_ERR_INVALID, "kern->gamma=%g must be finite and > 0 for VS_KTS_GRAM_RBF", kern->gamma);
    return VS_OK;
}

// the Gram launch's table for videos whose K lies at k_off[b] with row stride ldk[b]; appends its workspace at `off`
int plan_gram(const int32_t *cu, int32_t batch, Plan &P, int64_t off) {
    P.gvids.assign(batch, KtsGramVideo{});
    int64_t tiles = 0;
    for (int32_t b = 0; b < batch; ++b) {
        KtsGramVideo &G = P.gvids[b];
        G.n = cu[b + 1] - cu[b];
        G.row0 = cu[b];
        G.tile0 = (int32_t)tiles;
        const int64_t t = (G.n + KTS_GRAM_TILE - 1) / KTS_GRAM_TILE;
        tiles += t * (t + 1) / 2;
        if (tiles > INT32_MAX) return vs_failf(VS_ERR_INVALID, "the batch has more than 2^31 Gram tiles");
    }
    P.tiles = (int32_t)tiles;
    P.gvids_off = off; off = align256(off + (int64_t)batch * (int64_t)sizeof(KtsGramVideo));
    P.nrm_off = off; off = align256(off + (int64_t)cu[batch] * 8);
    P.total = off;
    return VS_OK;
}

// row norms (cosine / rbf), the table, the one Gram launch: all enqueued, nothing copied from host memory
int gram_k(const float *x, int32_t d, int32_t rows, const vs_kts_kernel &kern, const Plan &P, char *ws, void *kbase,
           hipStream_t st) {
    VS_LAUNCH(vsk_kts_put(P.gvids.data(), P.gvids.size() * sizeof(KtsGramVideo), ws + P.gvids_off, st));
    double *nrm = nullptr;
    if (kern.kind != VS_KTS_GRAM_DOT) {
        nrm = (double *)(ws + P.nrm_off);
        VS_LAUNCH(vsk_kts_row_norms(x, d, rows, kern.kind == VS_KTS_GRAM_COSINE, nrm, st));
    }
    VS_LAUNCH(vsk_kts_gram(x, d, (const KtsGramVideo *)(ws + P.gvids_off), (int)P.gvids.size(), P.tiles, kern.kind,
                            kern.gamma, nrm, kbase, st));
    return VS_OK;
}

// make_plan for a *_k entry point: features only, the Gram of every video where the scatter stage reads it
int make_plan_k(const int32_t *cu, int32_t batch, int32_t d, int32_t input, const int32_t *ncp, const int32_t *lmin,
                const int32_t *lmax, int32_t mode, const vs_kts_kernel *kern, Plan &P) {
    if (int rc = check_kernel(kern)) return rc;
    if (input == VS_KTS_KERNEL_F32 || input == VS_KTS_KERNEL_F64)
        return vs_failf(VS_ERR_INVALID, "a kernel-matrix input has its kernel already: kern needs VS_KTS_FEATURES_F32");
    if (int rc = make_plan(cu, batch, d, input, ncp, lmin, lmax, mode, P)) return rc;
    if (int rc = plan_gram(cu, batch, P, P.total)) return rc;
    for (int32_t b = 0; b < batch; ++b) {
        P.gvids[b].ldk = P.vids[b].ldk;
        P.gvids[b].k_off = P.vids[b].k_off;
    }
    return VS_OK;
}

// features -> scatter table through the one-launch Gram
int table_k(const float *x, int32_t d, const int32_t *cu, const vs_kts_kernel &kern, const Plan &P, char *ws, hipStream_t st) {
    const int B = (int)P.vids.size();
    VS_LAUNCH(vsk_kts_put(P.vids.data(), P.vids.size() * sizeof(KtsVideo), ws, st));
    if (int rc = gram_k(x, d, cu[B], kern, P, ws, ws, st)) return rc;
    VS_LAUNCH(vsk_kts_scatter_table((const KtsVideo *)ws, B, P.n_max, ws, ws, 0, st));
    return VS_OK;
}

// everything of vs_kts_segment after the scatter table: the dynamic program, the model selection, the back-tracking
int finish_segment(Plan &P, int32_t batch, const double *vmax, const double *desc_rate, int32_t mode, int64_t *cps,
                   int32_t *n_cps, double *scores, char *ws, hipStream_t st) {
    const KtsVideo *dv = (const KtsVideo *)ws;
    VS_LAUNCH(vsk_kts_dp_init(dv, batch, P.n_max, ws, st));
    for (int32_t k = 1; k <= P.m_max; ++k) VS_LAUNCH(vsk_kts_dp_step(dv, batch, P.n_max, k, ws, st));

    int64_t n_scores = 0, n_total_cps = 0;
    for (const KtsVideo &V : P.vids) { n_scores += V.m + 1; n_total_cps += V.m; }
    VS_HIP(hipMemcpyAsync(scores, ws + P.vids[0].s_off, (size_t)n_scores * 8, hipMemcpyDeviceToHost, st));
    VS_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n_scores; ++i)
        if (scores[i] > 1e99) scores[i] = INFINITY;           // scores[scores > 1e99] = np.inf

    if (mode == VS_KTS_AUTO) {                               // cpd_auto.py: penalty, costs, first argmin
        double *s = scores;
        for (int32_t b = 0; b < batch; ++b) {
            KtsVideo &V = P.vids[b];
            const double N = (double)V.n, N2 = N * (desc_rate ? desc_rate[b] : 1.0);
            int32_t best = 0;
            for (int32_t c = 0; c <= V.m; ++c) {
                const double pen = c == 0 ? 0.0 : (vmax[b] * (double)c / (2.0 * N2)) * (std::log(N2 / (double)c) + 1.0);
                s[c] = s[c] / N + pen;
                if (s[c] < s[best]) best = c;
            }
            if ((int64_t)V.n > (int64_t)(best + 1) * V.lmax)
                return vs_failf(VS_ERR_INVALID, "video %d: needs n <= (m_best + 1) * lmax (n=%d m_best=%d lmax=%d)", b, V.n, best,
                            V.lmax);
            V.mbest = best;
            s += V.m + 1;
        }
    }
    int64_t c_at = 0;
    if (mode == VS_KTS_SCORES) {
        for (int32_t b = 0; b < batch; ++b) n_cps[b] = P.vids[b].m;
        std::memset(cps, 0, (size_t)n_total_cps * sizeof(int64_t));
        return VS_OK;
    }
    if (int rc = upload(P, ws, st)) return rc;               // m_best
    VS_LAUNCH(vsk_kts_backtrack(dv, batch, ws, st));
    std::vector<int32_t> c32((size_t)n_total_cps + 1);
    VS_HIP(hipMemcpyAsync(c32.data(), ws + P.vids[0].c_off, (size_t)n_total_cps * 4, hipMemcpyDeviceToHost, st));
    VS_HIP(hipStreamSynchronize(st));
    for (int32_t b = 0; b < batch; ++b) {
        const KtsVideo &V = P.vids[b];
        n_cps[b] = V.mbest;
        for (int32_t i = 0; i < V.m; ++i) cps[c_at + i] = i < V.mbest ? (int64_t)c32[c_at + i] : 0;
        c_at += V.m;
    }
    return VS_OK;
}

}  // namespace

extern "C" {

size_t vs_kts_workspace_bytes(const int32_t *cu, int32_t batch, int32_t d, int32_t input, const int32_t *ncp, int32_t mode) {
    Plan P;
    if (make_plan(cu, batch, d, input, ncp, nullptr, nullptr, mode, P) != VS_OK) return 0;
    return (size_t)P.total;
}

int vs_kts_segment(const void *x, int32_t input, int32_t d, const int32_t *cu, int32_t batch, const int32_t *ncp,
                   const int32_t *lmin, const int32_t *lmax, const double *vmax, const double *desc_rate, int32_t mode,
                   int64_t *cps, int32_t *n_cps, double *scores, void *workspace, size_t workspace_bytes, void *stream) {
    Plan P;
    if (int rc = make_plan(cu, batch, d, input, ncp, lmin, lmax, mode, P)) return rc;
    if (!x || !cps || !n_cps || !scores) return vs_failf(VS_ERR_INVALID, "x / cps / n_cps / scores is NULL");
    if (mode == VS_KTS_AUTO) {
        if (!vmax) return vs_failf(VS_ERR_INVALID, "vmax is NULL (needed by VS_KTS_AUTO)");
        for (int32_t b = 0; b < batch; ++b)
            if (desc_rate && !(desc_rate[b] > 0)) return vs_failf(VS_ERR_INVALID, "video %d: desc_rate=%g must be > 0", b, desc_rate[b]);
    }
    if (!workspace || workspace_bytes < (size_t)P.total)
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %lld needed", workspace_bytes, (long long)P.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    if (int rc = table(x, input, d, cu, P, ws, st)) return rc;
    return finish_segment(P, batch, vmax, desc_rate, mode, cps, n_cps, scores, ws, st);
}

int vs_kts_scatters(const void *x, int32_t input, int32_t d, int32_t n, double *scatters, void *workspace,
                    size_t workspace_bytes, void *stream) {
    const int32_t cu[2] = {0, n}, zero = 0;
    Plan P;
    if (int rc = make_plan(cu, 1, d, input, &zero, nullptr, nullptr, VS_KTS_SCORES, P)) return rc;
    if (!x || !scatters) return vs_failf(VS_ERR_INVALID, "x / scatters is NULL");
    if (!workspace || workspace_bytes < (size_t)P.total)
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %lld needed", workspace_bytes, (long long)P.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    if (int rc = table(x, input, d, cu, P, ws, st)) return rc;
    VS_LAUNCH(vsk_kts_scatters_out((const KtsVideo *)ws, n, ws, scatters, st));
    VS_HIP(hipStreamSynchronize(st));                        // the plan's host copy of the descriptors ends here
    return VS_OK;
}

size_t vs_kts_gram_workspace_bytes(const int32_t *cu, int32_t batch, int32_t d) {
    const vs_kts_kernel dot = {VS_KTS_GRAM_DOT, 0, 0.0};
    Plan P;
    std::vector<int32_t> zeros(batch > 0 ? batch : 0, 0);
    if (!cu || batch <= 0) { vs_failf(VS_ERR_INVALID, "cu is NULL or batch=%d is not positive", batch); return 0; }
    if (make_plan_k(cu, batch, d, VS_KTS_FEATURES_F32, zeros.data(), nullptr, nullptr, VS_KTS_SCORES, &dot, P) != VS_OK)
        return 0;                                            // the same checks of cu / d as every other entry point
    if (plan_gram(cu, batch, P, 0) != VS_OK) return 0;
    return (size_t)P.total;
}

int vs_kts_gram(const void *x, int32_t d, const int32_t *cu, int32_t batch, const vs_kts_kernel *kern, float *K_out,
                void *workspace, size_t workspace_bytes, void *stream) {
    Plan P;
    if (!cu || batch <= 0) return vs_failf(VS_ERR_INVALID, "cu is NULL or batch=%d is not positive", batch);
    std::vector<int32_t> zeros(batch, 0);
    if (int rc = make_plan_k(cu, batch, d, VS_KTS_FEATURES_F32, zeros.data(), nullptr, nullptr, VS_KTS_SCORES, kern, P)) return rc;
    if (!x || !K_out) return vs_failf(VS_ERR_INVALID, "x / K_out is NULL");
    if (int rc = plan_gram(cu, batch, P, 0)) return rc;
    int64_t k_off = 0;
    for (int32_t b = 0; b < batch; ++b) {                    // dense, one video after the other
        KtsGramVideo &G = P.gvids[b];
        G.ldk = G.n;
        G.k_off = k_off;
        k_off += (int64_t)G.n * G.n * 4;
    }
    if (!workspace || workspace_bytes < (size_t)P.total)
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %lld needed", workspace_bytes, (long long)P.total);
    return gram_k((const float *)x, d, cu[batch], *kern, P, (char *)workspace, K_out, (hipStream_t)stream);
}

size_t vs_kts_workspace_bytes_k(const int32_t *cu, int32_t batch, int32_t d, int32_t input, const int32_t *ncp, int32_t mode,
                                const vs_kts_kernel *kern) {
    Plan P;
    if (make_plan_k(cu, batch, d, input, ncp, nullptr, nullptr, mode, kern, P) != VS_OK) return 0;
    return (size_t)P.total;
}

int vs_kts_segment_k(const void *x, int32_t input, int32_t d, const int32_t *cu, int32_t batch, const int32_t *ncp,
                     const int32_t *lmin, const int32_t *lmax, const double *vmax, const double *desc_rate, int32_t mode,
                     const vs_kts_kernel *kern, int64_t *cps, int32_t *n_cps, double *scores, void *workspace,
                     size_t workspace_bytes, void *stream) {
    Plan P;
    if (int rc = make_plan_k(cu, batch, d, input, ncp, lmin, lmax, mode, kern, P)) return rc;
    if (!x || !cps || !n_cps || !scores) return vs_failf(VS_ERR_INVALID, "x / cps / n_cps / scores is NULL");
    if (mode == VS_KTS_AUTO) {
        if (!vmax) return vs_failf(VS_ERR_INVALID, "vmax is NULL (needed by VS_KTS_AUTO)");
        for (int32_t b = 0; b < batch; ++b)
            if (desc_rate && !(desc_rate[b] > 0)) return vs_failf(VS_ERR_INVALID, "video %d: desc_rate=%g must be > 0", b, desc_rate[b]);
    }
    if (!workspace || workspace_bytes < (size_t)P.total)
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %lld needed", workspace_bytes, (long long)P.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    if (int rc = table_k((const float *)x, d, cu, *kern, P, ws, st)) return rc;
    return finish_segment(P, batch, vmax, desc_rate, mode, cps, n_cps, scores, ws, st);
}

int vs_kts_eval_score(const void *x, int32_t input, int32_t d, const vs_kts_kernel *kern, const int32_t *cu, int32_t batch,
                      const int64_t *cps, const int32_t *n_cps, double *scores_out, void *workspace, size_t workspace_bytes,
                      void *stream) {
    const vs_kts_kernel dot = {VS_KTS_GRAM_DOT, 0, 0.0};
    const bool feats = input == VS_KTS_FEATURES_F32;
    if (!n_cps) return vs_failf(VS_ERR_INVALID, "n_cps is NULL");
    Plan P;
    if (feats) {
        if (int rc = make_plan_k(cu, batch, d, input, n_cps, nullptr, nullptr, VS_KTS_SCORES, kern ? kern : &dot, P)) return rc;
    } else if (int rc = make_plan(cu, batch, d, input, n_cps, nullptr, nullptr, VS_KTS_SCORES, P)) {
        return rc;                                           // n_cps > n - 1 is refused here: n >= (ncp + 1) lmin
    }
    int64_t total_cps = 0;
    for (int32_t b = 0; b < batch; ++b) total_cps += n_cps[b];
    if (!x || !scores_out || (total_cps && !cps)) return vs_failf(VS_ERR_INVALID, "x / cps / scores_out is NULL");
    std::vector<int32_t> c32((size_t)total_cps + 1);
    int64_t at = 0;
    for (int32_t b = 0; b < batch; ++b) {
        const int32_t n = P.vids[b].n;
        int64_t prev = 0;
        for (int32_t i = 0; i < n_cps[b]; ++i, ++at) {
            const int64_t c = cps[at];
            if (c <= prev || c > n - 1)
                return vs_failf(VS_ERR_INVALID, "video %d: change point %d = %lld must be in 1 .. n - 1 = %d and above the one before it",
                            b, i, (long long)c, n - 1);
            c32[(size_t)at] = (int32_t)c;
            prev = c;
        }
    }
    if (!workspace || workspace_bytes < (size_t)P.total)
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %lld needed", workspace_bytes, (long long)P.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    if (feats) {
        if (int rc = table_k((const float *)x, d, cu, kern ? *kern : dot, P, ws, st)) return rc;
    } else if (int rc = table(x, input, d, cu, P, ws, st)) {
        return rc;
    }
    if (total_cps) VS_LAUNCH(vsk_kts_put(c32.data(), (size_t)total_cps * 4, ws + P.vids[0].c_off, st));
    VS_LAUNCH(vsk_kts_eval((const KtsVideo *)ws, batch, ws, st));
    // every video's s_off is (m + 1) doubles after the one before: gather the first of each on the host
    int64_t n_scores = 0;
    for (const KtsVideo &V : P.vids) n_scores += V.m + 1;
    std::vector<double> s((size_t)n_scores);
    VS_HIP(hipMemcpyAsync(s.data(), ws + P.vids[0].s_off, (size_t)n_scores * 8, hipMemcpyDeviceToHost, st));
    VS_HIP(hipStreamSynchronize(st));
    int64_t si = 0;
    for (int32_t b = 0; b < batch; ++b) {
        scores_out[b] = s[(size_t)si];
        si += P.vids[b].m + 1;
    }
    return VS_OK;
}

}  // extern "C"
