// Internal launcher interface between the KTS C ABI (vs_segment.cpp) and its kernels (vs_segment.hip).
// Every launcher enqueues on `st`, never synchronises, and returns 0 or a hipError_t.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One video of a KTS batch as the kernels see it.  Every *_off is a BYTE offset into the workspace `ws`, except k_off,
// which is a byte offset into the kernel-matrix base (the caller's K, or the Gram buffer inside the workspace).
struct KtsVideo {
    int32_t n, m, lmin, lmax;
    int32_t ldk;          // row stride of K in elements
    int32_t mbest;        // change points to back-track (set by the host before vsk_kts_backtrack)
    int64_t k_off;
    int64_t w_off;        // double [(n + 1)][(n + 1)]: 2-D prefix of K; its strict lower triangle becomes J by segment end
    int64_t t_off;        // double [ceil(n / KTS_CHUNK)][n + 1]: column totals of the row chunks
    int64_t k1_off;       // double [n + 1]: prefix of diag(K)
    int64_t i_off;        // double [2][n + 1]: the two rolling objective rows
    int64_t s_off;        // double [m + 1]: I[:, n]
    int64_t p_off;        // int32 [m + 1][n + 1] back-pointers, or -1 (scores only)
    int64_t c_off;        // int32 [m]: change points
};

enum { KTS_CHUNK = 64 };  // rows per chunk of the column scan

// K (float when kdouble == 0, else double) -> W = 2-D prefix, K1, then J in place.  n_max = max n of the batch.
int vsk_kts_scatter_table(const KtsVideo *vids, int B, int n_max, char *ws, const void *kbase, int kdouble, hipStream_t st);
// row 0 of the objective, then one dynamic-program step k over the batch (videos with m < k idle)
int vsk_kts_dp_init(const KtsVideo *vids, int B, int n_max, char *ws, hipStream_t st);
int vsk_kts_dp_step(const KtsVideo *vids, int B, int n_max, int k, char *ws, hipStream_t st);
// cps[0 .. mbest) from the back-pointers, one thread per video
int vsk_kts_backtrack(const KtsVideo *vids, int B, char *ws, hipStream_t st);
// out [n][n] = J in the reference's orientation (start row, end column), zeros below the diagonal; video 0 of vids
int vsk_kts_scatters_out(const KtsVideo *vids, int n, const char *ws, double *out, hipStream_t st);

// ---- vs_segment_gram.hip: the ragged-batch Gram with its kernel epilogue, and the score of given change points ----

// One video of a Gram launch.  tile0 = the videos' lower-triangle 64 x 64 tile counts summed over the earlier videos.
struct KtsGramVideo {
    int32_t n, row0;      // frames, first row in the packed x
    int32_t ldk, tile0;   // row stride of K in elements
    int64_t k_off;        // byte offset of K from the output base
};

enum { KTS_GRAM_TILE = 64 };

// bytes (a multiple of 4) of a host table -> device memory, carried by kernel arguments: stream-ordered, no host copy,
// and the host table may be freed as soon as this returns
int vsk_kts_put(const void *src, size_t bytes, void *dst, hipStream_t st);
// out[row] = sum_k x[row][k]^2 in double (inverse == 0), or 1 / sqrt of it, 0 for an all-zero row (inverse == 1)
int vsk_kts_row_norms(const float *x, int d, int rows, int inverse, double *out, hipStream_t st);
// K_v = epilogue(X_v X_v^T) of every video in one launch; kind: VS_KTS_GRAM_*; nrm: vsk_kts_row_norms output over all
// the rows of x (NULL for the dot kind); tiles = the batch's total tile count
int vsk_kts_gram(const float *x, int d, const KtsGramVideo *vids, int B, int tiles, int kind, double gamma,
                 const double *nrm, void *kbase, hipStream_t st);
// s_off[0] = sum of the scatters of the segments cut by the m change points at c_off, read from the scatter table
int vsk_kts_eval(const KtsVideo *vids, int B, char *ws, hipStream_t st);
