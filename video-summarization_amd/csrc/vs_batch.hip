// vs_batch.hip — the batches of a training epoch cut from a device-resident set (include/vs_batch.h): gather kernels for
// gfx950 and the C entries over them.
//
// The kernels are pure copies, so they are built for the HBM copy rate: a block owns one UNIT of the output at a time -
// UNIT_VECS 16-byte vectors, i.e. as many whole output rows as fit (4 rows of 1024 floats, 1024 rows of 4 floats) or, for
// rows wider than that, one UNIT_VECS-wide segment of one row.  Per unit the block first resolves the unit's rows - which
// video, hence which arena row; one binary search of `out_start` per ROW, not per vector - into LDS and copies the side
// value (and writes the mask) of those rows on the way; then every thread moves VECS vectors with the loads issued before
// the stores.  The grid is capped at MAX_BLOCKS and strides over the units; a unit's result depends on nothing but its
// index.  When the width is no multiple of 4 floats or a pointer is not 16-byte aligned the same code runs with 4-byte
// elements.
//
// Whatever the device arrays hold, stores stay inside the output the HOST integers describe and loads inside the arena:
// the search returns a slot in [0, B), ids are clamped to [0, V) and source rows to [0, video_start[V]).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "vs_batch.h"
#include "vs_error.h"
#include "vs_scorer.h"

namespace {

constexpr int NT = 256;                       // threads per block (4 waves)
constexpr int VECS = 4;                       // vectors per thread and unit
constexpr int UNIT_VECS = NT * VECS;          // 1024 vectors (16 KiB on the 16-byte path) per unit
constexpr int MAX_BLOCKS = 2048;              // 256 CUs x 8 resident blocks; more units are strided over

struct GatherArgs {
    const float *arena, *side;
    const int64_t *video_start;
    const int32_t *ids, *out_start;
    float *out, *side_out;
    uint8_t *mask_out;
    int64_t rows;                 // output rows: total_rows (packed) or B * t_max (padded)
    int32_t V, B, t_max, dv;      // dv: row width in vectors
    int32_t rows_per_unit, segs;  // whole rows per unit (dv <= UNIT_VECS) or segments per row (dv > UNIT_VECS)
    float pad;
};

typedef float vec4 __attribute__((ext_vector_type(4)));      // the 16-byte access type (a plain vector: it lives in registers)

template <typename T> __device__ __forceinline__ T splat(float x);
template <> __device__ __forceinline__ float splat<float>(float x) { return x; }
template <> __device__ __forceinline__ vec4 splat<vec4>(float x) { return vec4{x, x, x, x}; }

// arena row of output row r, or -1 for a padded row
template <bool PADDED>
__device__ __forceinline__ int64_t source_row(const GatherArgs &a, int64_t r, int64_t arena_rows) {
    int b;
    int64_t t;
    if (PADDED) {
        b = (int)(r / a.t_max);
        t = r - (int64_t)b * a.t_max;
        if (t >= (int64_t)a.out_start[b + 1] - a.out_start[b]) return -1;
    } else {
        int lo = 0, hi = a.B;                 // out_start[lo] <= r < out_start[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)a.out_start[mid] <= r) lo = mid; else hi = mid;
        }
        b = lo;
        t = r - a.out_start[b];
    }
    int id = a.ids[b];
    id = id < 0 ? 0 : (id >= a.V ? a.V - 1 : id);
    int64_t s = a.video_start[id] + t;
    if (s < 0) s = 0;
    if (s >= arena_rows) s = arena_rows - 1;      // arena_rows <= 0 (a corrupt video_start): -1, the row is written as padding
    return s;
}

template <typename T, bool PADDED>
__global__ __launch_bounds__(NT) void gather_rows_of_videos(const GatherArgs a) {
    __shared__ int64_t s_src[UNIT_VECS];
    const T *arena = reinterpret_cast<const T *>(a.arena);
    T *out = reinterpret_cast<T *>(a.out);
    const int64_t arena_rows = a.video_start[a.V];
    const int64_t row_groups = (a.rows + a.rows_per_unit - 1) / a.rows_per_unit;
    const int64_t units = row_groups * a.segs;
    const T padv = splat<T>(a.pad);
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t grp = u / a.segs;
        const int seg = (int)(u - grp * a.segs);
        const int64_t row0 = grp * a.rows_per_unit;
        const int nrows = (int)((a.rows - row0) < a.rows_per_unit ? (a.rows - row0) : a.rows_per_unit);
        const int col0 = seg * UNIT_VECS;
        const int ncols = (a.dv - col0) < UNIT_VECS ? (a.dv - col0) : UNIT_VECS;     // == dv when the unit holds whole rows
        for (int lr = threadIdx.x; lr < nrows; lr += NT) {
            const int64_t r = row0 + lr;
            const int64_t s = source_row<PADDED>(a, r, arena_rows);
            s_src[lr] = s;
            if (seg == 0) {
                if (a.side_out) a.side_out[r] = s < 0 ? a.pad : a.side[s];
                if (PADDED && a.mask_out) a.mask_out[r] = s < 0 ? 1 : 0;
            }
        }
        __syncthreads();
        const int nvec = nrows * ncols;       // <= UNIT_VECS
        T val[VECS];
#pragma unroll
        for (int k = 0; k < VECS; ++k) {
            const int j = threadIdx.x + k * NT;
            val[k] = padv;
            if (j < nvec) {
                const int lr = j / ncols;
                const int64_t s = s_src[lr];
                if (s >= 0) val[k] = arena[s * a.dv + col0 + (j - lr * ncols)];
            }
        }
#pragma unroll
        for (int k = 0; k < VECS; ++k) {
            const int j = threadIdx.x + k * NT;
            if (j < nvec) {
                const int lr = j / ncols;
                out[(row0 + lr) * a.dv + col0 + (j - lr * ncols)] = val[k];
            }
        }
        __syncthreads();                      // s_src is rewritten by the next unit
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void gather_table_rows(const float *table_, int32_t n_rows, const int32_t *ids, int64_t total,
                                                        int32_t wv, float *out_) {
    const T *table = reinterpret_cast<const T *>(table_);
    T *out = reinterpret_cast<T *>(out_);
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int64_t b = i / wv;
        int id = ids[b];
        id = id < 0 ? 0 : (id >= n_rows ? n_rows - 1 : id);
        out[i] = table[(int64_t)id * wv + (i - b * wv)];
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

int check_common(const char *fn, const float *arena, const float *side, const int64_t *video_start, int32_t n_videos,
                 const int32_t *ids, const int32_t *out_start, int32_t B, int32_t d, const float *out, const float *side_out) {
    if (!arena || !video_start || !ids || !out_start || !out)
        return vs_failf(VS_ERR_INVALID, "%s: arena / video_start / ids / out_start / out is NULL", fn);
    if ((side == nullptr) != (side_out == nullptr))
        return vs_failf(VS_ERR_INVALID, "%s: side and side_out go together, one of them is NULL", fn);
    if (n_videos < 1) return vs_failf(VS_ERR_INVALID, "%s: n_videos=%d (>= 1)", fn, n_videos);
    if (B < 1) return vs_failf(VS_ERR_INVALID, "%s: B=%d (>= 1)", fn, B);
    if (d < 1) return vs_failf(VS_ERR_INVALID, "%s: d=%d (>= 1)", fn, d);
    return VS_OK;
}

template <bool PADDED>
int launch_gather(GatherArgs a, int32_t d, void *stream) {
    const bool vec = d % 4 == 0 && aligned16(a.arena) && aligned16(a.out);
    a.dv = vec ? d / 4 : d;
    a.rows_per_unit = a.dv >= UNIT_VECS ? 1 : UNIT_VECS / a.dv;
    a.segs = a.dv > UNIT_VECS ? (a.dv + UNIT_VECS - 1) / UNIT_VECS : 1;
    const int64_t units = (a.rows + a.rows_per_unit - 1) / a.rows_per_unit * a.segs;
    const unsigned grid = (unsigned)(units < MAX_BLOCKS ? units : MAX_BLOCKS);
    if (vec) hipLaunchKernelGGL((gather_rows_of_videos<vec4, PADDED>), dim3(grid), dim3(NT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((gather_rows_of_videos<float, PADDED>), dim3(grid), dim3(NT), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vs_failf(VS_ERR_HIP, "batch gather launch failed: %s", hipGetErrorString(e));
    return VS_OK;
}

}  // namespace

extern "C" {

int vs_batch_gather_packed(const float *arena, const float *side_or_null, const int64_t *video_start, int32_t n_videos,
                           const int32_t *ids, const int32_t *out_start, int32_t B, int64_t total_rows, int32_t d,
                           float *out, float *side_out_or_null, void *stream) {
    if (int rc = check_common("vs_batch_gather_packed", arena, side_or_null, video_start, n_videos, ids, out_start, B, d, out,
                              side_out_or_null))
        return rc;
    if (total_rows < B || total_rows >= ((int64_t)1 << 31))
        return vs_failf(VS_ERR_INVALID, "vs_batch_gather_packed: total_rows=%lld for B=%d videos (every video has a row; < 2^31)",
                     (long long)total_rows, B);
    GatherArgs a{};
    a.arena = arena; a.side = side_or_null; a.video_start = video_start; a.ids = ids; a.out_start = out_start;
    a.out = out; a.side_out = side_out_or_null; a.mask_out = nullptr;
    a.rows = total_rows; a.V = n_videos; a.B = B; a.t_max = 0; a.pad = 0.0f;
    return launch_gather<false>(a, d, stream);
}

int vs_batch_gather_padded(const float *arena, const float *side_or_null, const int64_t *video_start, int32_t n_videos,
                           const int32_t *ids, const int32_t *out_start, int32_t B, int32_t longest, int32_t t_max,
                           float pad_value, int32_t d, float *out, float *side_out_or_null, uint8_t *mask_out_or_null,
                           void *stream) {
    if (int rc = check_common("vs_batch_gather_padded", arena, side_or_null, video_start, n_videos, ids, out_start, B, d, out,
                              side_out_or_null))
        return rc;
    if (longest < 1) return vs_failf(VS_ERR_INVALID, "vs_batch_gather_padded: longest=%d (>= 1)", longest);
    if (t_max < longest)
        return vs_failf(VS_ERR_INVALID, "vs_batch_gather_padded: t_max=%d is below the longest video of the batch (%d frames)", t_max,
                     longest);
    GatherArgs a{};
    a.arena = arena; a.side = side_or_null; a.video_start = video_start; a.ids = ids; a.out_start = out_start;
    a.out = out; a.side_out = side_out_or_null; a.mask_out = mask_out_or_null;
    a.rows = (int64_t)B * t_max; a.V = n_videos; a.B = B; a.t_max = t_max; a.pad = pad_value;
    return launch_gather<true>(a, d, stream);
}

int vs_batch_gather_rows(const float *table, int32_t n_rows, const int32_t *ids, int32_t B, int32_t w, float *out,
                         void *stream) {
    if (!table || !ids || !out) return vs_failf(VS_ERR_INVALID, "vs_batch_gather_rows: table / ids / out is NULL");
    if (n_rows < 1) return vs_failf(VS_ERR_INVALID, "vs_batch_gather_rows: n_rows=%d (>= 1)", n_rows);
    if (B < 1) return vs_failf(VS_ERR_INVALID, "vs_batch_gather_rows: B=%d (>= 1)", B);
    if (w < 1) return vs_failf(VS_ERR_INVALID, "vs_batch_gather_rows: w=%d (>= 1)", w);
    const bool vec = w % 4 == 0 && aligned16(table) && aligned16(out);
    const int32_t wv = vec ? w / 4 : w;
    const int64_t total = (int64_t)B * wv;
    const int64_t blocks = (total + NT - 1) / NT;
    const unsigned grid = (unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
    if (vec) hipLaunchKernelGGL(gather_table_rows<vec4>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, table, n_rows, ids, total, wv, out);
    else hipLaunchKernelGGL(gather_table_rows<float>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, table, n_rows, ids, total, wv, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vs_failf(VS_ERR_HIP, "vs_batch_gather_rows launch failed: %s", hipGetErrorString(e));
    return VS_OK;
}

}  // extern "C"
