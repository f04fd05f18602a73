// vs_cnn3d_plan.h - the R3D-18 video-level feature as data: the 20 conv records of one forward in execution
// order, where each reads, writes and takes its residual from, the workspace they need - a pure function of (N, T, H, W).
// vs_cnn3d.cpp only walks the plan.  The gather's and the store's address arithmetic (cnn3d_pos / cnn3d_tap / cnn3d_offset /
// cnn3d_store_offset) is written here once: conv3d_igemm (vs_cnn3d.hip) calls the same four functions for every element it loads
// or stores.  Host code, plain C++17, no HIP include and no globals: tests/cabi/cnn3d_plan_demo.cpp compiles this header alone.
//
// The network accepts every T, H, W >= 1: a 3 x 3 x 3 conv of pad 1 and stride s, the stem's 7 x 7 of pad 3 and stride 2 and a
// 1 x 1 x 1 conv of stride 2 all give floor((in - 1) / s) + 1 >= 1 outputs per dimension, so no layer is ever empty and the plan
// states no smallest side (torch agrees: tests/r3d_ref.py runs at 1 x 1 x 1).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VS_CNN3D_HD __host__ __device__
#else
#define VS_CNN3D_HD
#endif

enum { CNN3D_TILE_M = 64, CNN3D_TILE_N = 64, CNN3D_TILE_K = 32 };       // conv3d_igemm's tile: rows (positions) x columns (Cout) x k-step
enum { CNN3D_NUM_CONVS = 20, CNN3D_FEATURES = 512 };
enum { CNN3D_IN_F32_NCDHW = 0, CNN3D_IN_U8_NDHWC = 1, CNN3D_IN_F32_NDHWC = 2 };  // = VS_CNN3D_INPUT_* of vs_video_features.h
// workspace buffers: 0 / 1 the blocks' ping-pong, 2 conv1's output, 3 the downsample's output
enum { CNN3D_BUF_INPUT = -1, CNN3D_BUF_NONE = -3, CNN3D_NUM_BUFS = 4 };

// ---- one convolution as an implicit GEMM: rows = N*To*Ho*Wo positions, columns = Cout, k = (kt, kh, kw, cin) ascending ----
struct Cnn3dConv {
    int32_t N, T, H, W, Cin, Cout;
    int32_t kt, ks, st, ss, pt, ps;     // temporal / spatial kernel size, stride, padding
    int32_t To, Ho, Wo;
    int32_t K, Kp, Coutp;               // kt*ks*ks*Cin; padded to the k-step; Cout padded to the column tile
    int64_t M;                          // N*To*Ho*Wo
    int64_t sn, sd, sh, sw, sc;         // element strides of the input: video, frame, row, column, channel
};

struct Cnn3dPos { int64_t base; int32_t ti0, hi0, wi0; bool valid; };   // output position m: its video's offset and its first tap
struct Cnn3dTap { int32_t dt, dh, dw, c; bool valid; };                 // k: its tap and its channel

VS_CNN3D_HD inline Cnn3dPos cnn3d_pos(const Cnn3dConv &g, int64_t m) {
    Cnn3dPos px{0, 0, 0, 0, false};
    if (m < 0 || m >= g.M) return px;                                   // row guard: the last row tile is partial
    const int64_t hw = (int64_t)g.Ho * g.Wo, thw = hw * g.To, n = m / thw;
    const int32_t r = (int32_t)(m - n * thw), to = r / (int32_t)hw, q = r - to * (int32_t)hw, ho = q / g.Wo, wo = q - ho * g.Wo;
    px.base = n * g.sn; px.ti0 = to * g.st - g.pt; px.hi0 = ho * g.ss - g.ps; px.wi0 = wo * g.ss - g.ps; px.valid = true;
    return px;
}

VS_CNN3D_HD inline Cnn3dTap cnn3d_tap(const Cnn3dConv &g, int32_t k) {
    Cnn3dTap t{0, 0, 0, 0, false};
    if (k < 0 || k >= g.K) return t;                                    // k padding: the packed weights hold zeros there
    const int32_t tap = k / g.Cin, ss = g.ks * g.ks;
    t.c = k - tap * g.Cin; t.dt = tap / ss;
    const int32_t q = tap - t.dt * ss;
    t.dh = q / g.ks; t.dw = q - t.dh * g.ks; t.valid = true;
    return t;
}

// element offset of (position, tap) in the input, or -1 where the tap is padding in time or space (it reads as zero), k >= K or m >= M
VS_CNN3D_HD inline int64_t cnn3d_offset(const Cnn3dConv &g, const Cnn3dPos &px, const Cnn3dTap &t) {
    if (!px.valid || !t.valid) return -1;
    const int32_t ti = px.ti0 + t.dt, hi = px.hi0 + t.dh, wi = px.wi0 + t.dw;
    if (ti < 0 || ti >= g.T || hi < 0 || hi >= g.H || wi < 0 || wi >= g.W) return -1;
    return px.base + ti * g.sd + hi * g.sh + wi * g.sw + t.c * g.sc;
}

// element offset of output (m, col) in the channels-last destination (and in the residual, which has its shape), or -1 (row / column guard)
VS_CNN3D_HD inline int64_t cnn3d_store_offset(const Cnn3dConv &g, int64_t m, int32_t col) {
    if (m < 0 || m >= g.M || col < 0 || col >= g.Cout) return -1;
    return m * g.Cout + col;
}

inline int32_t cnn3d_round_up(int32_t v, int32_t to) { return (v + to - 1) / to * to; }
inline int32_t cnn3d_conv_out(int32_t in, int32_t k, int32_t s, int32_t p) {
    const int64_t a = (int64_t)in + 2 * p - k;
    return a < 0 ? 0 : (int32_t)(a / s) + 1;
}

// fills the derived fields; layout: CNN3D_IN_* (the NDHWC forms are dense in Cin)
inline Cnn3dConv cnn3d_conv_geometry(int32_t N, int32_t T, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t kt, int32_t ks, int32_t st,
                                     int32_t ss, int32_t pt, int32_t ps, int32_t layout) {
    Cnn3dConv g{};
    g.N = N; g.T = T; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.kt = kt; g.ks = ks; g.st = st; g.ss = ss; g.pt = pt; g.ps = ps;
    g.To = cnn3d_conv_out(T, kt, st, pt); g.Ho = cnn3d_conv_out(H, ks, ss, ps); g.Wo = cnn3d_conv_out(W, ks, ss, ps);
    g.K = kt * ks * ks * Cin; g.Kp = cnn3d_round_up(g.K, CNN3D_TILE_K); g.Coutp = cnn3d_round_up(Cout, CNN3D_TILE_N);
    g.M = (int64_t)N * g.To * g.Ho * g.Wo;
    if (layout == CNN3D_IN_F32_NCDHW) { g.sw = 1; g.sh = W; g.sd = (int64_t)H * W; g.sc = g.sd * T; g.sn = g.sc * Cin; }
    else { g.sc = 1; g.sw = Cin; g.sh = (int64_t)W * Cin; g.sd = g.sh * H; g.sn = g.sd * T; }
    return g;
}
inline int64_t cnn3d_packed_weight_floats(const Cnn3dConv &g) { return (int64_t)g.Coutp * g.Kp; }
inline int64_t cnn3d_flops(const Cnn3dConv &g) { return 2 * g.M * g.K * g.Cout; }      // of the convolution as stated, padding taps included

// ---- the records ----
struct Cnn3dConvRec {
    Cnn3dConv g;
    int32_t in_buf, out_buf, res_buf, relu;     // CNN3D_BUF_INPUT or a workspace buffer; res_buf CNN3D_BUF_NONE: no residual
    int64_t w_off, b_off;                       // floats into the packed blob: weights [Coutp][Kp], then bias [Coutp]
};
struct Cnn3dPlan {
    bool ok;
    const char *why;
    int32_t N, T, H, W;
    Cnn3dConvRec conv[CNN3D_NUM_CONVS];
    int32_t pool_buf;                           // the final mean: over pool_positions = T'*H'*W' per (n, channel) of this buffer
    int64_t pool_positions;
    int64_t buf_off[CNN3D_NUM_BUFS], buf_floats[CNN3D_NUM_BUFS];    // floats, each offset a multiple of 64 (256 bytes)
    int64_t blob_floats, workspace_bytes, flops;
};

// The whole forward for N videos of T frames of H x W.  input_layout: CNN3D_IN_F32_NCDHW or CNN3D_IN_U8_NDHWC (the stem's gather).
// Record order = execution order = the order of vs_r3d_params: stem, then per block of layer1..layer4: conv1, downsample (first
// block of layer2..4 only), conv2.  conv2 adds the block's identity (its input, or the downsample's output) and applies the final
// ReLU in its epilogue.  plan.ok == false (plan.why says what) when a row count leaves int32.
inline Cnn3dPlan cnn3d_make_plan(int32_t N, int32_t T, int32_t H, int32_t W, int32_t input_layout) {
    Cnn3dPlan P{};
    P.N = N; P.T = T; P.H = H; P.W = W; P.ok = false;
    if (N < 1 || T < 1 || H < 1 || W < 1) { P.why = "n, t, h or w below 1"; return P; }
    if (input_layout != CNN3D_IN_F32_NCDHW && input_layout != CNN3D_IN_U8_NDHWC) { P.why = "unknown input kind"; return P; }
    if ((int64_t)N * T * H * W > (int64_t)1 << 30) { P.why = "more than 2^30 input positions: a row count would leave int32"; return P; }
    int nc = 0, t = T, h = H, w = W;
    int64_t blob = 0;
    auto conv = [&](int in_buf, int cin, int cout, int kt, int ks, int st, int ss, int pt, int ps, int out_buf, int res_buf, int relu, int layout) {
        Cnn3dConvRec &R = P.conv[nc++];
        R.g = cnn3d_conv_geometry(N, t, h, w, cin, cout, kt, ks, st, ss, pt, ps, layout);
        R.in_buf = in_buf; R.out_buf = out_buf; R.res_buf = res_buf; R.relu = relu;
        R.w_off = blob; blob += cnn3d_packed_weight_floats(R.g);
        R.b_off = blob; blob += R.g.Coutp;
        if (R.g.M * cout > P.buf_floats[out_buf]) P.buf_floats[out_buf] = R.g.M * cout;
        P.flops += cnn3d_flops(R.g);
        return &R.g;
    };
    int cur = 0, c = 64;
    {
        const Cnn3dConv *g = conv(CNN3D_BUF_INPUT, 3, 64, 3, 7, 1, 2, 1, 3, cur, CNN3D_BUF_NONE, 1, input_layout);
        t = g->To; h = g->Ho; w = g->Wo;
    }
    for (int layer = 0; layer < 4; ++layer) {
        const int planes = 64 << layer;
        for (int block = 0; block < 2; ++block) {
            const int s = (layer > 0 && block == 0) ? 2 : 1, nxt = cur ^ 1;
            const Cnn3dConv *g1 = conv(cur, c, planes, 3, 3, s, s, 1, 1, 2, CNN3D_BUF_NONE, 1, CNN3D_IN_F32_NDHWC);
            int res = cur;
            if (s == 2) { conv(cur, c, planes, 1, 1, 2, 2, 0, 0, 3, CNN3D_BUF_NONE, 0, CNN3D_IN_F32_NDHWC); res = 3; }
            t = g1->To; h = g1->Ho; w = g1->Wo; c = planes;
            conv(2, c, planes, 3, 3, 1, 1, 1, 1, nxt, res, 1, CNN3D_IN_F32_NDHWC);
            cur = nxt;
        }
    }
    P.pool_buf = cur;
    P.pool_positions = (int64_t)t * h * w;
    int64_t off = 0;
    for (int b = 0; b < CNN3D_NUM_BUFS; ++b) { P.buf_off[b] = off; off += (P.buf_floats[b] + 63) / 64 * 64; }
    P.blob_floats = blob;
    P.workspace_bytes = off * 4;
    P.ok = nc == CNN3D_NUM_CONVS && c == CNN3D_FEATURES;
    if (!P.ok) P.why = "internal: the record count is off";
    return P;
}
