// vs_cnn_plan.h - the GoogLeNet pool5 front end as data: the 57 conv records and 14 pool records of one
// forward, where each reads and writes, the workspace they need, and the smallest frame the network accepts - a pure function of
// (N, H, W).  vs_cnn.cpp only walks the plan.  The gather's address arithmetic (cnn_pixel / cnn_tap / cnn_offset) is written
// here once: conv_igemm (vs_cnn.hip) calls the same three functions for every element it loads.
// Host code, plain C++17, no HIP include and no globals: tests/cabi/cnn_plan_demo.cpp compiles this header alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VS_CNN_HD __host__ __device__
#else
#define VS_CNN_HD
#endif

enum { CNN_TILE_M = 64, CNN_TILE_N = 64, CNN_TILE_K = 32 };        // conv_igemm's tile: rows (pixels) x columns (Cout) x k-step
enum { CNN_NUM_CONVS = 57, CNN_NUM_POOLS = 14, CNN_NUM_STEPS = CNN_NUM_CONVS + CNN_NUM_POOLS, CNN_FEATURES = 1024 };
enum { CNN_IN_F32_NCHW = 0, CNN_IN_U8_NHWC = 1, CNN_IN_F32_NHWC = 2 };       // = VS_CNN_INPUT_* of vs_features.h
enum { CNN_BUF_INPUT = -1, CNN_BUF_OUTPUT = -2, CNN_NUM_BUFS = 5 };          // 0 / 1 ping-pong, 2..4 an Inception block's branch temporaries

// ---- one convolution as an implicit GEMM: rows = N*Ho*Wo pixels, columns = Cout, k = (kh, kw, cin) ascending ----
struct CnnConv {
    int32_t N, H, W, Cin, Cout, k, s, p, Ho, Wo;
    int32_t K, Kp, Coutp;           // k*k*Cin; padded to the k-step; Cout padded to the column tile
    int64_t M;                      // N*Ho*Wo
    int64_t sn, sh, sw, sc;         // element strides of the input: frame, row, column, channel
};

struct CnnPixel { int64_t base; int32_t hi0, wi0; bool valid; };   // output pixel m: its frame's offset and its first tap
struct CnnTap { int32_t dh, dw, c; bool valid; };                  // k: its tap and its channel

VS_CNN_HD inline CnnPixel cnn_pixel(const CnnConv &g, int64_t m) {
    CnnPixel px{0, 0, 0, false};
    if (m < 0 || m >= g.M) return px;                               // row guard: the last row tile is partial
    const int64_t hw = (int64_t)g.Ho * g.Wo, n = m / hw;
    const int32_t r = (int32_t)(m - n * hw), ho = r / g.Wo, wo = r - ho * g.Wo;
    px.base = n * g.sn; px.hi0 = ho * g.s - g.p; px.wi0 = wo * g.s - g.p; px.valid = true;
    return px;
}

VS_CNN_HD inline CnnTap cnn_tap(const CnnConv &g, int32_t k) {
    CnnTap t{0, 0, 0, false};
    if (k < 0 || k >= g.K) return t;                                // k padding: the packed weights hold zeros there
    const int32_t tap = k / g.Cin;
    t.c = k - tap * g.Cin; t.dh = tap / g.k; t.dw = tap - t.dh * g.k; t.valid = true;
    return t;
}

// element offset of (pixel, tap) in the input, or -1 where the tap is padding (it reads as zero), k >= K or m >= M
VS_CNN_HD inline int64_t cnn_offset(const CnnConv &g, const CnnPixel &px, const CnnTap &t) {
    if (!px.valid || !t.valid) return -1;
    const int32_t hi = px.hi0 + t.dh, wi = px.wi0 + t.dw;
    if (hi < 0 || hi >= g.H || wi < 0 || wi >= g.W) return -1;
    return px.base + hi * g.sh + wi * g.sw + t.c * g.sc;
}

// element offset of output (m, col) in a destination of row stride ldc written from channel c0, or -1 (row / column guard)
VS_CNN_HD inline int64_t cnn_store_offset(const CnnConv &g, int64_t m, int32_t col, int32_t c0, int32_t ldc) {
    if (m < 0 || m >= g.M || col < 0 || col >= g.Cout) return -1;
    return m * ldc + c0 + col;
}

inline int32_t cnn_round_up(int32_t v, int32_t to) { return (v + to - 1) / to * to; }
inline int64_t cnn_floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
inline int32_t cnn_conv_out(int32_t in, int32_t k, int32_t s, int32_t p) { return (int32_t)cnn_floor_div((int64_t)in + 2 * p - k, s) + 1; }
// torch's pooling_output_shape: with ceil_mode the last window must start inside the input or its left padding
inline int32_t cnn_pool_out(int32_t in, int32_t k, int32_t s, int32_t p, int32_t ceil_mode) {
    int32_t out = (int32_t)cnn_floor_div((int64_t)in + 2 * p - k + (ceil_mode ? s - 1 : 0), s) + 1;
    if (ceil_mode && (int64_t)(out - 1) * s >= (int64_t)in + p) --out;
    return out;
}

// fills the derived fields; layout: CNN_IN_* (the NHWC forms are dense in Cin)
inline CnnConv cnn_conv_geometry(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t k, int32_t s, int32_t p, int32_t layout) {
    CnnConv g{};
    g.N = N; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.k = k; g.s = s; g.p = p;
    g.Ho = cnn_conv_out(H, k, s, p); g.Wo = cnn_conv_out(W, k, s, p);
    g.K = k * k * Cin; g.Kp = cnn_round_up(g.K, CNN_TILE_K); g.Coutp = cnn_round_up(Cout, CNN_TILE_N);
    g.M = (int64_t)N * g.Ho * g.Wo;
    if (layout == CNN_IN_F32_NCHW) { g.sn = (int64_t)Cin * H * W; g.sc = (int64_t)H * W; g.sh = W; g.sw = 1; }
    else { g.sn = (int64_t)H * W * Cin; g.sh = (int64_t)W * Cin; g.sw = Cin; g.sc = 1; }
    return g;
}
inline int64_t cnn_packed_weight_floats(const CnnConv &g) { return (int64_t)g.Coutp * g.Kp; }

// ---- the records ----
struct CnnConvRec {
    CnnConv g;
    int32_t in_buf, out_buf, c0, ldc;       // CNN_BUF_INPUT or a workspace buffer; the destination's channel offset and row stride
    int64_t w_off, b_off;                   // floats into the packed blob: weights [Coutp][Kp], then bias [Coutp]
};
struct CnnPoolRec {
    int32_t avg, N, H, W, C, k, s, p, ceil_mode, Ho, Wo, in_buf, out_buf;   // avg: the mean over H*W into [N, C]
};
struct CnnStep { int32_t pool, index; };    // execution order over both tables
struct CnnPlan {
    bool ok;
    const char *why;
    int32_t N, H, W;
    CnnConvRec conv[CNN_NUM_CONVS];
    CnnPoolRec pool[CNN_NUM_POOLS];
    CnnStep step[CNN_NUM_STEPS];
    int64_t buf_off[CNN_NUM_BUFS], buf_floats[CNN_NUM_BUFS];        // floats, each offset a multiple of 64 (256 bytes)
    int64_t blob_floats, workspace_bytes;
};

struct CnnInception { int32_t in, c1, c3r, c3, c5r, c5, pp; };
inline const CnnInception *cnn_inceptions() {
    static const CnnInception t[9] = {{192, 64, 96, 128, 16, 32, 32},    {256, 128, 128, 192, 32, 96, 64},  {480, 192, 96, 208, 16, 48, 64},
                                      {512, 160, 112, 224, 24, 64, 64},  {512, 128, 128, 256, 24, 64, 64},  {512, 112, 144, 288, 32, 64, 64},
                                      {528, 256, 160, 320, 32, 128, 128}, {832, 256, 160, 320, 32, 128, 128}, {832, 384, 192, 384, 48, 128, 128}};
    return t;
}

// The whole forward for N frames of H x W.  input_layout: CNN_IN_F32_NCHW or CNN_IN_U8_NHWC (conv1's gather).
// Conv order = parameter order: conv1, conv2, conv3, then per Inception block branch1, branch2.0, branch2.1, branch3.0,
// branch3.1, branch4.1.  plan.ok == false (plan.why says what) when a layer would have no output or a count leaves int32.
inline CnnPlan cnn_make_plan(int32_t N, int32_t H, int32_t W, int32_t input_layout) {
    CnnPlan P{};
    P.N = N; P.H = H; P.W = W; P.ok = false;
    if (N < 1 || H < 1 || W < 1) { P.why = "n, h or w below 1"; return P; }
    if (input_layout != CNN_IN_F32_NCHW && input_layout != CNN_IN_U8_NHWC) { P.why = "unknown input kind"; return P; }
    int nc = 0, np = 0, ns = 0, cur = 0, h = H, w = W, c = 3;
    int64_t blob = 0;
    bool bad = false;
    auto need = [&](int buf, int64_t floats) { if (buf >= 0 && floats > P.buf_floats[buf]) P.buf_floats[buf] = floats; };
    auto conv = [&](int in_buf, int hh, int ww, int cin, int cout, int k, int s, int p, int out_buf, int c0, int ldc, int layout) {
        CnnConvRec &R = P.conv[nc];
        R.g = cnn_conv_geometry(N, hh, ww, cin, cout, k, s, p, layout);
        R.in_buf = in_buf; R.out_buf = out_buf; R.c0 = c0; R.ldc = ldc;
        R.w_off = blob; blob += cnn_packed_weight_floats(R.g);
        R.b_off = blob; blob += R.g.Coutp;
        if (R.g.Ho < 1 || R.g.Wo < 1 || R.g.M > (int64_t)1 << 30) bad = true;     // rows stay inside int32 with room for the tile
        else need(out_buf, R.g.M * ldc);
        P.step[ns++] = CnnStep{0, nc++};
        return &R.g;
    };
    auto pool = [&](int avg, int in_buf, int hh, int ww, int cc, int k, int s, int p, int ceil_mode, int out_buf) {
        CnnPoolRec &R = P.pool[np];
        R = CnnPoolRec{avg, N, hh, ww, cc, k, s, p, ceil_mode, avg ? 1 : cnn_pool_out(hh, k, s, p, ceil_mode),
                       avg ? 1 : cnn_pool_out(ww, k, s, p, ceil_mode), in_buf, out_buf};
        if (R.Ho < 1 || R.Wo < 1) bad = true;
        else need(out_buf, (int64_t)N * R.Ho * R.Wo * cc);
        P.step[ns++] = CnnStep{1, np++};
        return &R;
    };
    auto max_pool = [&](int k, int s) {
        const CnnPoolRec *R = pool(0, cur, h, w, c, k, s, 0, 1, cur ^ 1);
        h = R->Ho; w = R->Wo; cur ^= 1;
    };
    auto inception = [&](const CnnInception &I) {
        const int out = I.c1 + I.c3 + I.c5 + I.pp, dst = cur ^ 1;
        conv(cur, h, w, c, I.c1, 1, 1, 0, dst, 0, out, CNN_IN_F32_NHWC);
        conv(cur, h, w, c, I.c3r, 1, 1, 0, 2, 0, I.c3r, CNN_IN_F32_NHWC);
        conv(2, h, w, I.c3r, I.c3, 3, 1, 1, dst, I.c1, out, CNN_IN_F32_NHWC);
        conv(cur, h, w, c, I.c5r, 1, 1, 0, 3, 0, I.c5r, CNN_IN_F32_NHWC);
        conv(3, h, w, I.c5r, I.c5, 3, 1, 1, dst, I.c1 + I.c3, out, CNN_IN_F32_NHWC);
        pool(0, cur, h, w, c, 3, 1, 1, 1, 4);
        conv(4, h, w, c, I.pp, 1, 1, 0, dst, I.c1 + I.c3 + I.c5, out, CNN_IN_F32_NHWC);
        c = out; cur = dst;
    };
    const CnnInception *I = cnn_inceptions();
    {
        const CnnConv *g = conv(CNN_BUF_INPUT, h, w, 3, 64, 7, 2, 3, cur, 0, 64, input_layout);
        h = g->Ho; w = g->Wo; c = 64;
    }
    if (!bad) max_pool(3, 2);
    if (!bad) { conv(cur, h, w, 64, 64, 1, 1, 0, cur ^ 1, 0, 64, CNN_IN_F32_NHWC); cur ^= 1; }
    if (!bad) { conv(cur, h, w, 64, 192, 3, 1, 1, cur ^ 1, 0, 192, CNN_IN_F32_NHWC); cur ^= 1; c = 192; }
    if (!bad) max_pool(3, 2);
    for (int i = 0; i < 2 && !bad; ++i) inception(I[i]);
    if (!bad) max_pool(3, 2);
    for (int i = 2; i < 7 && !bad; ++i) inception(I[i]);
    if (!bad) max_pool(2, 2);
    for (int i = 7; i < 9 && !bad; ++i) inception(I[i]);
    if (bad) { P.why = "a layer would have no output (h or w too small) or the batch is too large"; return P; }
    pool(1, cur, h, w, c, 0, 1, 0, 0, CNN_BUF_OUTPUT);
    int64_t off = 0;
    for (int b = 0; b < CNN_NUM_BUFS; ++b) { P.buf_off[b] = off; off += (P.buf_floats[b] + 63) / 64 * 64; }
    P.blob_floats = blob;
    P.workspace_bytes = off * 4;
    P.ok = nc == CNN_NUM_CONVS && np == CNN_NUM_POOLS && c == CNN_FEATURES;
    if (!P.ok) P.why = "internal: the record count is off";
    return P;
}

// the smallest side the network accepts (the same for H and W): found by asking the plan, not stated twice
inline int32_t cnn_min_side() {
    static const int32_t side = [] { int32_t s = 1; while (!cnn_make_plan(1, s, s, CNN_IN_F32_NCHW).ok) ++s; return s; }();
    return side;
}
