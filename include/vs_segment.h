/*
 * vs_segment.h — C ABI of kernel temporal segmentation (KTS): shot boundaries of a video from its frame features.
 * Replaces the reference's segmentations/kts (cpd_nonlin.py: calc_scatters, cpd_nonlin; cpd_auto.py:
 * kts_segmentation) and the "kts" branch of create_segments.py (kts_seg: K = X X^T, no normalisation).
 *
 * Stages (all on the GPU, one stream): Gram K = X X^T in fp32 on the matrix pipe, the diagonal and 2-D prefix sums of K
 * in fp64, the scatter table J in fp64, then the change-point dynamic program - one launch per number of change points k
 * over the whole ragged batch, fp64 add and compare, ties to the smallest split.  Only the (ncp + 1) objective values
 * and the change points come back to the host; the model-selection penalty and its argmin are host arithmetic in
 * double.  Device pointers: x, workspace, scatters.  Host pointers: cu and every per-video parameter and output.
 * Every function returns 0 or a VS_ERR_* status (vs_scorer.h) and sets vs_last_error(); the argument checks need no
 * GPU.  Both entry points synchronise `stream` before they return.
 */
#ifndef VS_SEGMENT_H
#define VS_SEGMENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* what x holds */
#define VS_KTS_FEATURES_F32 0  /* frame features, float [cu[batch]][d], any d >= 1; K = X X^T is computed here */
#define VS_KTS_KERNEL_F32 1    /* the videos' kernel matrices, float, video v = n_v * n_v values after those of v - 1 */
#define VS_KTS_KERNEL_F64 2    /* the same in double */

/* what vs_kts_segment returns */
#define VS_KTS_SCORES 0        /* cpd_nonlin(backtrack=False): scores; the change points are zeros, n_cps = ncp */
#define VS_KTS_BACKTRACK 1     /* cpd_nonlin(backtrack=True): scores and the ncp change points */
#define VS_KTS_AUTO 2          /* kts_segmentation: costs (scores / n + penalty) and the change points of the best count */

/* Device bytes vs_kts_segment needs for this batch (0: invalid arguments, see vs_last_error()).  The dominant term is
 * (n + 1)^2 doubles per video: the prefix table that the scatter table overwrites in place (800 MB at n = 10 000);
 * then n * round_up(n, 32) floats of K when x is features, and (ncp + 1) (n + 1) int32 back-pointers unless mode is
 * VS_KTS_SCORES.  cu: host [batch + 1] frame offsets, cu[0] = 0. */
size_t vs_kts_workspace_bytes(const int32_t *cu, int32_t batch, int32_t d, int32_t input, const int32_t *ncp, int32_t mode);

/* Replaces: kts_segmentation(K, ncp, vmax, desc_rate, lmin=, lmax=) (mode VS_KTS_AUTO) and cpd_nonlin(K, ncp, lmin, lmax,
 * backtrack) (modes VS_KTS_SCORES / VS_KTS_BACKTRACK) for every video of a ragged batch at once.
 * x: device, see `input`; d: feature width (ignored for the kernel inputs).
 * ncp, lmin, lmax: host [batch]; lmin / lmax may be NULL (1 / 100000).  vmax, desc_rate: host [batch] doubles, read in
 * mode VS_KTS_AUTO only (desc_rate may be NULL: 1).  The reference's asserts are VS_ERR_INVALID: n >= (ncp + 1) lmin,
 * n <= (ncp + 1) lmax, lmax >= lmin >= 1, and in mode VS_KTS_AUTO also n <= (m_best + 1) lmax.
 * Outputs (host): scores [sum (ncp_v + 1)] doubles, video v after those of v - 1, unreachable entries +inf (costs in
 * mode VS_KTS_AUTO); cps [sum ncp_v] change points, video v at offset sum_{u<v} ncp_u, n_cps [batch] of them valid. */
int vs_kts_segment(const void *x, int32_t input, int32_t d, const int32_t *cu, int32_t batch, const int32_t *ncp,
                   const int32_t *lmin, const int32_t *lmax, const double *vmax, const double *desc_rate, int32_t mode,
                   int64_t *cps, int32_t *n_cps, double *scores, void *workspace, size_t workspace_bytes, void *stream);

/* Replaces: calc_scatters(K) (the out_scatters of cpd_nonlin) for one video of n frames.  scatters: device double
 * [n][n], scatters[i][j] = scatter of frames i..j for j >= i, 0 below the diagonal.  workspace: at least
 * vs_kts_workspace_bytes({0, n}, 1, d, input, {0}, VS_KTS_SCORES) bytes.  Synchronises `stream`. */
int vs_kts_scatters(const void *x, int32_t input, int32_t d, int32_t n, double *scatters, void *workspace,
                    size_t workspace_bytes, void *stream);

/* ---- cosine and Gaussian kernels; the Gram of a ragged batch in one launch --------------------------------------------
 * x is float [n][d].  g_ij = the fp32 matrix-pipe dot product of rows i and j (the fma chain over k ascending),
 * s_i = sum_k x_ik^2 accumulated in double in a fixed order.
 *   DOT:    K_ij = g_ij.
 *   COSINE: inv_i = s_i > 0 ? 1 / sqrt(s_i) : 0 (double); K_ij = float(clamp((double)g_ij * inv_i * inv_j, -1, 1)) for
 *           i != j; K_ii = s_i > 0 ? 1 : 0.  An all-zero frame has a zero row and column.
 *   RBF:    K_ij = float(exp(-gamma * max(0, s_i + s_j - 2 (double)g_ij))), exp in double; K_ii = 1.
 * K is symmetric bit for bit (both halves are stored from one accumulator), and a video's K does not depend on the
 * videos it is batched with, on its place among them, or on the call. */
#define VS_KTS_GRAM_DOT 0
#define VS_KTS_GRAM_COSINE 1
#define VS_KTS_GRAM_RBF 2

typedef struct vs_kts_kernel {
    int32_t kind;      /* VS_KTS_GRAM_* */
    int32_t reserved;  /* 0 */
    double gamma;      /* RBF only: finite and > 0; ignored by the other kinds */
} vs_kts_kernel;

/* Device bytes vs_kts_gram needs (0: invalid arguments, see vs_last_error()). */
size_t vs_kts_gram_workspace_bytes(const int32_t *cu, int32_t batch, int32_t d);

/* The kernel matrices of a ragged batch: one row-norm pre-pass (cosine / rbf) and ONE Gram launch for all videos, operands
 * read straight from x (no padded copy).  x: device float [cu[batch]][d]; cu: host [batch + 1]; kern: host.
 * K_out: device float, video v = n_v * n_v dense values after those of v - 1 - the VS_KTS_KERNEL_F32 input layout.
 * Stream-ordered: enqueues on `stream` and returns; no copy to or from host memory, no synchronisation. */
int vs_kts_gram(const void *x, int32_t d, const int32_t *cu, int32_t batch, const vs_kts_kernel *kern, float *K_out,
                void *workspace, size_t workspace_bytes, void *stream);

/* vs_kts_workspace_bytes / vs_kts_segment with the kernel of the Gram chosen by `kern` (host, not NULL).  Same contracts
 * otherwise; `input` must be VS_KTS_FEATURES_F32 (a kernel matrix has its kernel already: VS_ERR_INVALID).  The Gram
 * comes from the one-launch kernel above for all three kinds.  kind = VS_KTS_GRAM_DOT here computes the same g_ij as
 * vs_kts_segment where the fp32 Gram is exact; on data whose fp32 Gram rounds it is NOT bound to vs_kts_segment's bits
 * (that path sums a zero-padded copy on another GEMM's tiling). */
size_t vs_kts_workspace_bytes_k(const int32_t *cu, int32_t batch, int32_t d, int32_t input, const int32_t *ncp, int32_t mode,
                                const vs_kts_kernel *kern);
int vs_kts_segment_k(const void *x, int32_t input, int32_t d, const int32_t *cu, int32_t batch, const int32_t *ncp,
                     const int32_t *lmin, const int32_t *lmax, const double *vmax, const double *desc_rate, int32_t mode,
                     const vs_kts_kernel *kern, int64_t *cps, int32_t *n_cps, double *scores, void *workspace,
                     size_t workspace_bytes, void *stream);

/* Replaces: eval_score(K, cps) (cpd_auto.py) for every video of a ragged batch: the sum of the scatters of the segments
 * that the given change points cut, each scatter evaluated as the scatter table of vs_kts_segment evaluates it and added
 * left to right in double - the additions of the dynamic program along that path, so the value is bit-equal to the
 * cpd_nonlin score of its own change points.  x / input / d as vs_kts_segment; kern (host, NULL = DOT) chooses the
 * kernel of a VS_KTS_FEATURES_F32 input and is ignored for the two kernel-matrix inputs.  cps: host int64, video v's
 * n_cps[v] change points after those of v - 1 (strictly increasing, in 1 .. n_v - 1, else VS_ERR_INVALID); n_cps: host
 * [batch].  scores_out: host double [batch].  workspace: at least vs_kts_workspace_bytes_k(cu, batch, d, input, n_cps,
 * VS_KTS_SCORES, kern) bytes (vs_kts_workspace_bytes for a kernel-matrix input is enough).  Synchronises `stream`. */
int vs_kts_eval_score(const void *x, int32_t input, int32_t d, const vs_kts_kernel *kern, const int32_t *cu, int32_t batch,
                      const int64_t *cps, const int32_t *n_cps, double *scores_out, void *workspace, size_t workspace_bytes,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VS_SEGMENT_H */
