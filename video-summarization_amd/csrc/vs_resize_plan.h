// vs_resize_plan.h - the frame resize as data and address arithmetic: the output-size rule, one axis'
// fixed-point coefficient table (PIL's antialiased bilinear for 8-bit images, restated), the tile geometry the kernel runs with,
// and every address the kernel forms for a load, an LDS access or a store.  resize_bilinear_u8 (vs_resize.hip) calls the same
// functions for every byte it moves; vs_resize.cpp chooses the tile once, here, on the host.
// Host code, plain C++17, no HIP include and no globals: tests/cabi/resize_plan_demo.cpp compiles this header alone.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <vector>

#if defined(__HIPCC__)
#define VS_RESIZE_HD __host__ __device__
#else
#define VS_RESIZE_HD
#endif

enum { RESIZE_PRECISION_BITS = 22 };
enum { RESIZE_THREADS = 256 };
// LDS of one block, sized per plan: the rounded intermediate (rows of the horizontal pass's output), the tile's coefficients, and
// one chunk of raw input rows.  All of it stays within RESIZE_LDS_BYTES (no opt-in to large LDS); the raw chunk takes what is left
// of RESIZE_LDS_TARGET (several blocks per CU; the intermediate alone may take RESIZE_MID_MAX), but at least RESIZE_RAW_MIN where the budget allows and at most RESIZE_RAW_MAX.
enum { RESIZE_LDS_BYTES = 65536, RESIZE_LDS_TARGET = 32768, RESIZE_MID_MAX = 32768, RESIZE_RAW_MIN = 8192, RESIZE_RAW_MAX = 24576 };
enum { RESIZE_TILE_OH = 32, RESIZE_TILE_OW = 64 };                  // the default tile of output rows x output columns
enum { RESIZE_PATH_FUSED = 0, RESIZE_PATH_SMALL_TILE = 1 };         // = VS_RESIZE_PATH_* of vs_resize.h
enum { RESIZE_MAX_SIDE = 1 << 16 };                                 // either side of either image

// ---- the output size: torchvision's rule for an int size (the shorter side becomes size; w <= h counts as "w is shorter") ----
inline bool resize_output_size(int32_t h, int32_t w, int32_t size, int32_t *oh, int32_t *ow) {
    if (h < 1 || w < 1 || size < 1 || h > RESIZE_MAX_SIDE || w > RESIZE_MAX_SIDE || size > RESIZE_MAX_SIDE) return false;
    const int64_t shorter = w <= h ? w : h, longer = w <= h ? h : w;
    const int64_t new_long = (int64_t)((double)((int64_t)size * longer) / (double)shorter);    // Python's int(size * long / short)
    if (new_long < 1 || new_long > RESIZE_MAX_SIDE) return false;
    if (w <= h) { *ow = size; *oh = (int32_t)new_long; }
    else { *oh = size; *ow = (int32_t)new_long; }
    return true;
}

// ---- one axis' table ----
// The doubles below must be the same whatever the compiler: no multiply-add may be contracted.  `center` stays a named variable,
// the translation units that include this for the tables are built with -ffp-contract=off, and clang is told here as well.
inline int32_t resize_ksize(int32_t in, int32_t out) {
    const double scale = (double)(float)in / out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    return (int32_t)ceil(support) * 2 + 1;
}

struct ResizeAxis {
    int32_t in, out, ksize;
    bool identity;                  // in == out: the pass is skipped (one tap of weight 1, which reproduces the byte exactly)
    std::vector<int32_t> bounds;    // [out][2]: xmin, n
    std::vector<int32_t> coef;      // [out][ksize]: fixed point, slots n .. ksize-1 are 0
};

// skip_equal: in == out gives the skipped pass (one tap of weight 1) instead of the filter's own table for that size
inline ResizeAxis resize_build_axis(int32_t in, int32_t out, bool skip_equal = true) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    ResizeAxis A;
    A.in = in; A.out = out; A.identity = skip_equal && in == out;
    if (A.identity) {
        A.ksize = 1;
        A.bounds.resize((size_t)out * 2);
        A.coef.assign((size_t)out, 1 << RESIZE_PRECISION_BITS);
        for (int32_t xx = 0; xx < out; ++xx) { A.bounds[2 * xx] = xx; A.bounds[2 * xx + 1] = 1; }
        return A;
    }
    const double scale = (double)(float)in / out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const int32_t ksize = (int32_t)ceil(support) * 2 + 1;
    A.ksize = ksize;
    A.bounds.assign((size_t)out * 2, 0);
    A.coef.assign((size_t)out * ksize, 0);
    std::vector<double> w((size_t)ksize);
    for (int32_t xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        const double ss = 1.0 / filterscale;
        int32_t xmin = (int32_t)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int32_t xmax = (int32_t)(center + support + 0.5);
        if (xmax > in) xmax = in;
        const int32_t n = xmax - xmin;
        double ww = 0.0;
        for (int32_t x = 0; x < n; ++x) {
            const double a = fabs((x + xmin - center + 0.5) * ss);
            w[x] = a < 1.0 ? 1.0 - a : 0.0;
            ww += w[x];
        }
        for (int32_t x = 0; x < n; ++x) {
            if (ww != 0.0) w[x] /= ww;
            const double scaled = w[x] * (double)(1 << RESIZE_PRECISION_BITS);
            A.coef[(size_t)xx * ksize + x] = w[x] < 0.0 ? (int32_t)(-0.5 + scaled) : (int32_t)(0.5 + scaled);
        }
        A.bounds[2 * xx] = xmin;
        A.bounds[2 * xx + 1] = n;
    }
    return A;
}

// ---- the geometry the kernel runs with ----
struct ResizeGeom {
    int32_t H, W, OH, OW;
    int32_t kx, ky;                 // taps per output column / row in the tables (1: that pass is skipped)
    int32_t tile_oh, tile_ow, tiles_y, tiles_x;
    int32_t raw_stride, raw_rows;   // bytes of one staged input row (a multiple of 4), input rows per chunk
    int32_t mid_stride, mid_rows;   // bytes of one intermediate row (a multiple of 4), the most input rows any tile reads
    int32_t raw_off, xk_off, yk_off, lds_bytes;     // LDS bytes: the intermediate at 0, then the raw chunk, the x and y coefficients
    int32_t lane_shift;             // log2(tile_ow): a thread's column inside the tile is tid & (tile_ow - 1), its row tid >> lane_shift
    int32_t path;                   // RESIZE_PATH_*
};

// output rows [oy0, oy1) x columns [ox0, ox1) of one frame; they read input rows [r0, r1) and input columns [c0, c1)
struct ResizeTile { int32_t oy0, oy1, ox0, ox1, r0, r1, c0, c1; };

// xmin and xmin + n do not decrease along an axis (center grows, the clamps keep order), so a tile's first and last window bound it
VS_RESIZE_HD inline void resize_span(const int32_t *bounds, int32_t o0, int32_t o1, int32_t *lo, int32_t *hi) {
    *lo = bounds[2 * o0];
    *hi = bounds[2 * (o1 - 1)] + bounds[2 * (o1 - 1) + 1];
}

VS_RESIZE_HD inline ResizeTile resize_tile(const ResizeGeom &g, const int32_t *xb, const int32_t *yb, int32_t tile) {
    ResizeTile t;
    const int32_t ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    t.oy0 = ty * g.tile_oh; t.oy1 = t.oy0 + g.tile_oh < g.OH ? t.oy0 + g.tile_oh : g.OH;
    t.ox0 = tx * g.tile_ow; t.ox1 = t.ox0 + g.tile_ow < g.OW ? t.ox0 + g.tile_ow : g.OW;
    resize_span(yb, t.oy0, t.oy1, &t.r0, &t.r1);
    resize_span(xb, t.ox0, t.ox1, &t.c0, &t.c1);
    return t;
}

VS_RESIZE_HD inline int64_t resize_frame_bytes(int32_t h, int32_t w) { return (int64_t)h * w * 3; }
// byte offset, inside its frame, of pixel (row, col)
VS_RESIZE_HD inline int64_t resize_pixel_offset(int32_t width, int32_t row, int32_t col) { return ((int64_t)row * width + col) * 3; }

// bytes a staged row of `seg` segment bytes takes: the segment lands at the phase of its global address (0..3), so that
// aligned global dwords are aligned LDS dwords, and the horizontal pass reads one dword past the last pixel's
VS_RESIZE_HD inline int32_t resize_raw_stride(int32_t seg) { return (seg + 6) / 4 * 4 + 4; }
VS_RESIZE_HD inline int32_t resize_raw_slots(int32_t phase, int32_t seg) { return (phase + seg + 3) / 4; }

// Stage A, one aligned dword slot j of a staged row: it holds segment bytes [4j - phase, 4j - phase + 4), of which
// [first, first + count) exist.  count == 4: one dword load at segment offset `seg_off` (aligned, because the segment's address
// minus its phase is); otherwise byte loads.  The LDS byte offset inside the staged row is 4j.
struct ResizeSlot { int32_t seg_off, lds_off, first, count; };
VS_RESIZE_HD inline ResizeSlot resize_load_slot(int32_t phase, int32_t seg, int32_t j) {
    ResizeSlot s;
    s.seg_off = 4 * j - phase;
    s.lds_off = 4 * j;
    s.first = s.seg_off < 0 ? -s.seg_off : 0;
    const int32_t end = seg - s.seg_off < 4 ? seg - s.seg_off : 4;
    s.count = end > s.first ? end - s.first : 0;
    return s;
}

// Stage B, tap `col` (an input column in [c0, c1)) of a staged row: the pixel's first byte is at `byte` of the staged row; the
// kernel reads the aligned dwords at byte & ~3 and (byte & ~3) + 4 and shifts by 8 * (byte & 3)
VS_RESIZE_HD inline int32_t resize_raw_byte(int32_t phase, int32_t c0, int32_t col) { return phase + 3 * (col - c0); }
// ... and where the rounded pixel goes: byte offset in the intermediate of (input row, output column)
VS_RESIZE_HD inline int32_t resize_mid_offset(const ResizeGeom &g, const ResizeTile &t, int32_t row, int32_t ocol) {
    return (row - t.r0) * g.mid_stride + 3 * (ocol - t.ox0);
}

// Stage C, dword j of an output row's segment inside the tile: intermediate bytes [4j, 4j + 4) of each tap's row, and output
// bytes [4j, 4j + count) of the segment
VS_RESIZE_HD inline int32_t resize_out_dwords(const ResizeTile &t) { return ((t.ox1 - t.ox0) * 3 + 3) / 4; }
VS_RESIZE_HD inline int32_t resize_store_count(const ResizeTile &t, int32_t j) {
    const int32_t left = (t.ox1 - t.ox0) * 3 - 4 * j;
    return left < 4 ? (left > 0 ? left : 0) : 4;
}
VS_RESIZE_HD inline int32_t resize_mid_dword(const ResizeGeom &g, const ResizeTile &t, int32_t row, int32_t j) {
    return (row - t.r0) * (g.mid_stride / 4) + j;
}

// one tap: pixel byte x coefficient.  Coefficients are in [0, 2^22] (resize_make_plan refuses a table outside [0, 2^24)), so the
// 24-bit multiplier gives the int32 product exactly
VS_RESIZE_HD inline uint32_t resize_mul(uint32_t byte, uint32_t coef) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(byte, coef);
#else
    return byte * coef;
#endif
}

VS_RESIZE_HD inline int32_t resize_clip8(int32_t acc) {
    const int32_t v = acc >> RESIZE_PRECISION_BITS;
    return v < 0 ? 0 : v > 255 ? 255 : v;
}

// ---- the choice of the tile, once, on the host ----
// The default tile where its input rows fit the staging; otherwise the largest smaller one that fits (fewer output rows first,
// then fewer columns): a 20x vertical reduction or 4K input shrink the tile instead of leaving the chip.  ok == false when even
// one output pixel's windows do not fit (a reduction of several thousand to one).  Tile widths are powers of two (lane_shift).
struct ResizePlanHost {
    bool ok;
    const char *why;
    ResizeGeom g;
    ResizeAxis x, y;
};

inline bool resize_fit(ResizeGeom &g, const ResizeAxis &x, const ResizeAxis &y) {
    g.tiles_y = (g.OH + g.tile_oh - 1) / g.tile_oh;
    g.tiles_x = (g.OW + g.tile_ow - 1) / g.tile_ow;
    g.mid_stride = (g.tile_ow * 3 + 3) / 4 * 4;
    g.lane_shift = 0;
    while ((1 << g.lane_shift) < g.tile_ow) ++g.lane_shift;
    int32_t rows = 0, cols = 0, lo, hi;
    for (int32_t ty = 0; ty < g.tiles_y; ++ty) {
        const int32_t o0 = ty * g.tile_oh, o1 = o0 + g.tile_oh < g.OH ? o0 + g.tile_oh : g.OH;
        resize_span(y.bounds.data(), o0, o1, &lo, &hi);
        if (hi - lo > rows) rows = hi - lo;
    }
    for (int32_t tx = 0; tx < g.tiles_x; ++tx) {
        const int32_t o0 = tx * g.tile_ow, o1 = o0 + g.tile_ow < g.OW ? o0 + g.tile_ow : g.OW;
        resize_span(x.bounds.data(), o0, o1, &lo, &hi);
        if (hi - lo > cols) cols = hi - lo;
    }
    g.mid_rows = rows;
    g.raw_stride = resize_raw_stride(cols * 3);
    const int64_t mid_bytes = (int64_t)rows * g.mid_stride;
    const int64_t coef_bytes = ((int64_t)g.tile_ow * g.kx + (int64_t)g.tile_oh * g.ky) * 4;
    if (mid_bytes > RESIZE_MID_MAX || mid_bytes + coef_bytes + g.raw_stride > RESIZE_LDS_BYTES) return false;
    int64_t budget = RESIZE_LDS_TARGET - mid_bytes - coef_bytes;
    if (budget < RESIZE_RAW_MIN) budget = RESIZE_RAW_MIN;
    if (budget > RESIZE_RAW_MAX) budget = RESIZE_RAW_MAX;
    if (budget > RESIZE_LDS_BYTES - mid_bytes - coef_bytes) budget = RESIZE_LDS_BYTES - mid_bytes - coef_bytes;
    g.raw_rows = (int32_t)(budget / g.raw_stride);
    if (g.raw_rows < 1) g.raw_rows = 1;
    if (g.raw_rows > rows) g.raw_rows = rows;
    g.raw_off = (int32_t)mid_bytes;
    g.xk_off = g.raw_off + g.raw_rows * g.raw_stride;
    g.yk_off = g.xk_off + g.tile_ow * g.kx * 4;
    g.lds_bytes = g.yk_off + g.tile_oh * g.ky * 4;
    return g.lds_bytes <= RESIZE_LDS_BYTES;
}

inline ResizePlanHost resize_make_plan(int32_t h, int32_t w, int32_t oh, int32_t ow) {
    ResizePlanHost P{};
    P.ok = false;
    if (h < 1 || w < 1 || oh < 1 || ow < 1) { P.why = "a size is below 1"; return P; }
    if (h > RESIZE_MAX_SIDE || w > RESIZE_MAX_SIDE || oh > RESIZE_MAX_SIDE || ow > RESIZE_MAX_SIDE) { P.why = "a side is above 65536"; return P; }
    P.x = resize_build_axis(w, ow);
    P.y = resize_build_axis(h, oh);
    for (const ResizeAxis *A : {&P.x, &P.y})
        for (const int32_t c : A->coef)
            if (c < 0 || c >= 1 << 24) { P.why = "internal: a coefficient is outside [0, 2^24)"; return P; }
    ResizeGeom &g = P.g;
    g.H = h; g.W = w; g.OH = oh; g.OW = ow; g.kx = P.x.ksize; g.ky = P.y.ksize;
    for (int32_t tw = RESIZE_TILE_OW; tw >= 1; tw /= 4)
        for (int32_t th = RESIZE_TILE_OH; th >= 1; th /= 2) {
            g.tile_oh = th; g.tile_ow = tw;
            if (!resize_fit(g, P.x, P.y)) continue;
            g.path = th == RESIZE_TILE_OH && tw == RESIZE_TILE_OW ? RESIZE_PATH_FUSED : RESIZE_PATH_SMALL_TILE;
            P.ok = true;
            return P;
        }
    P.why = "the reduction is too large: one output pixel's input rows or columns do not fit the LDS staging";
    return P;
}
