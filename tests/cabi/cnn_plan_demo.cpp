// csrc/vs_cnn_plan.h alone, as plain C++17 (no HIP): tests/test_cnn_plan_host.py builds this with the host compiler and
// -fsanitize=address,undefined.  For each (N, H, W) on the command line it makes the plan and walks it with the functions the
// kernel itself calls (cnn_pixel / cnn_tap / cnn_offset / cnn_store_offset), over the whole padded tile grid of every conv:
//   - every gather address is inside what the producer wrote (a 16-byte load where the kernel would issue one), every padding
//     tap, every k >= K and every row >= M reads nothing; every store address is inside its buffer and inside its own channels;
//   - the workspace buffers are disjoint, no step reads the buffer it writes, and every buffer a step reads holds, in all of its
//     channels, the tensor that step expects (so no live tensor was overwritten);
//   - every pool window holds at least one input pixel.
// It prints one line per trunk layer, "layer <channels> <h> <w>", for the test to compare with torch's own sizes, then "OK".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vs_cnn_plan.h"

#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAILED line %d: %s\n", __LINE__, #__VA_ARGS__); return 1; } } while (0)

namespace {

struct Tensor {                     // what a workspace buffer holds
    int64_t frames = 0, h = 0, w = 0, ld = 0;
    std::vector<char> written;      // per channel
    bool holds(int64_t n, int64_t hh, int64_t ww, int64_t c) const {
        if (frames != n || h != hh || w != ww || ld != c) return false;
        for (char x : written)
            if (!x) return false;
        return true;
    }
};

int walk(int32_t N, int32_t H, int32_t W, int32_t layout) {
    const CnnPlan P = cnn_make_plan(N, H, W, layout);
    CHECK(P.ok);
    // the buffers: in order, disjoint, 256-byte aligned, inside the workspace
    for (int b = 0; b < CNN_NUM_BUFS; ++b) {
        CHECK(P.buf_off[b] % 64 == 0 && P.buf_floats[b] > 0);
        const int64_t end = P.buf_off[b] + P.buf_floats[b];
        CHECK(end <= (b + 1 < CNN_NUM_BUFS ? P.buf_off[b + 1] : P.workspace_bytes / 4));
    }
    Tensor T[CNN_NUM_BUFS];
    int64_t blob_at = 0;
    int convs = 0, pools = 0;
    for (int s = 0; s < CNN_NUM_STEPS; ++s) {
        if (!P.step[s].pool) {
            CHECK(P.step[s].index == convs);
            const CnnConvRec &R = P.conv[convs++];
            const CnnConv &g = R.g;
            CHECK(g.N == N && g.K == g.k * g.k * g.Cin && g.Kp % CNN_TILE_K == 0 && g.Kp >= g.K && g.Kp - g.K < CNN_TILE_K);
            CHECK(g.Coutp % CNN_TILE_N == 0 && g.Coutp >= g.Cout && g.Coutp - g.Cout < CNN_TILE_N && g.M == (int64_t)N * g.Ho * g.Wo);
            CHECK(R.w_off == blob_at && R.b_off == R.w_off + (int64_t)g.Coutp * g.Kp);
            blob_at = R.b_off + g.Coutp;
            int64_t in_floats;
            bool vec4;
            if (R.in_buf == CNN_BUF_INPUT) {
                CHECK(s == 0 && g.Cin == 3 && g.H == H && g.W == W);
                in_floats = (int64_t)N * 3 * H * W;
                vec4 = false;
            } else {
                CHECK(R.in_buf >= 0 && R.in_buf < CNN_NUM_BUFS && R.in_buf != R.out_buf);
                CHECK(T[R.in_buf].holds(N, g.H, g.W, g.Cin));
                in_floats = (int64_t)N * g.H * g.W * g.Cin;
                CHECK(in_floats <= P.buf_floats[R.in_buf]);
                vec4 = true;
                CHECK(g.Cin % 4 == 0 && g.sc == 1 && g.sw == g.Cin);      // every layer but conv1 takes the 16-byte gather
            }
            // the gather, over the padded rows of the tile grid: first and last channel of every tap, and the k padding
            const int64_t Mp = (g.M + CNN_TILE_M - 1) / CNN_TILE_M * CNN_TILE_M;
            const int span = vec4 ? 4 : 1;
            for (int64_t m = 0; m < Mp; ++m) {
                const CnnPixel px = cnn_pixel(g, m);
                CHECK(px.valid == (m < g.M));
                int64_t n_inside = 0;
                for (int tap = 0; tap < g.k * g.k; ++tap) {
                    const int ks[2] = {tap * g.Cin, tap * g.Cin + g.Cin - span};
                    for (int k : ks) {
                        const CnnTap tp = cnn_tap(g, k);
                        CHECK(tp.valid && tp.dh == tap / g.k && tp.dw == tap % g.k && tp.c == k - tap * g.Cin);
                        const int64_t off = cnn_offset(g, px, tp);
                        const int hi = px.hi0 + tp.dh, wi = px.wi0 + tp.dw;
                        const bool inside = px.valid && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
                        CHECK((off >= 0) == inside);
                        if (inside) {
                            CHECK(off + span <= in_floats);
                            if (vec4) CHECK(off % 4 == 0);
                            ++n_inside;
                        }
                    }
                }
                if (px.valid) CHECK(n_inside > 0);                 // every output pixel sees the input
                for (int k = g.K; k < g.Kp; ++k) CHECK(cnn_offset(g, px, cnn_tap(g, k)) == -1);
            }
            CHECK(!cnn_tap(g, -1).valid && !cnn_pixel(g, -1).valid);
            // the stores: every row with the columns at the guards, every column with the rows at the guards
            CHECK(R.out_buf >= 0 && R.out_buf < CNN_NUM_BUFS && R.c0 >= 0 && R.c0 + g.Cout <= R.ldc);
            auto store_ok = [&](int64_t m, int col) {
                const int64_t off = cnn_store_offset(g, m, col, R.c0, R.ldc);
                if ((off >= 0) != (m < g.M && col < g.Cout)) return false;
                if (off < 0) return true;
                return off < P.buf_floats[R.out_buf] && off % R.ldc >= R.c0 && off % R.ldc < R.c0 + g.Cout && off / R.ldc == m;
            };
            const int cols[4] = {0, g.Cout - 1, g.Cout, g.Coutp - 1};
            for (int64_t m = 0; m < Mp; ++m)
                for (int col : cols) CHECK(store_ok(m, col));
            const int64_t rows[4] = {0, g.M - 1, g.M, Mp - 1};
            for (int col = 0; col < g.Coutp; ++col)
                for (int64_t m : rows) CHECK(store_ok(m, col));
            Tensor &D = T[R.out_buf];
            if (R.c0 == 0) { D.frames = N; D.h = g.Ho; D.w = g.Wo; D.ld = R.ldc; D.written.assign((size_t)R.ldc, 0); }
            CHECK(D.frames == N && D.h == g.Ho && D.w == g.Wo && D.ld == R.ldc);          // a later branch joins the same tensor
            for (int c = R.c0; c < R.c0 + g.Cout; ++c) { CHECK(!D.written[(size_t)c]); D.written[(size_t)c] = 1; }
            if (R.c0 == 0 && R.out_buf < 2) std::printf("layer %d %d %d\n", R.ldc, g.Ho, g.Wo);
        } else {
            CHECK(P.step[s].index == pools);
            const CnnPoolRec &R = P.pool[pools++];
            CHECK(R.N == N && R.in_buf >= 0 && R.in_buf < CNN_NUM_BUFS && R.in_buf != R.out_buf && R.C % 4 == 0);
            CHECK(T[R.in_buf].holds(N, R.H, R.W, R.C));
            if (R.avg) {
                CHECK(s == CNN_NUM_STEPS - 1 && R.out_buf == CNN_BUF_OUTPUT && R.C == CNN_FEATURES);
                std::printf("layer %d 1 1\n", R.C);
                continue;
            }
            CHECK(R.out_buf >= 0 && R.out_buf < CNN_NUM_BUFS && (int64_t)N * R.Ho * R.Wo * R.C <= P.buf_floats[R.out_buf]);
            for (int o = 0; o < R.Ho; ++o) CHECK(o * R.s - R.p < R.H && o * R.s - R.p + R.k > 0);     // a window is never empty
            for (int o = 0; o < R.Wo; ++o) CHECK(o * R.s - R.p < R.W && o * R.s - R.p + R.k > 0);
            CHECK((R.Ho - 1) * R.s - R.p + R.k >= R.H - (R.s - 1) && (R.Wo - 1) * R.s - R.p + R.k >= R.W - (R.s - 1));   // nothing but a stride's rest is left over
            Tensor &D = T[R.out_buf];
            D.frames = N; D.h = R.Ho; D.w = R.Wo; D.ld = R.C; D.written.assign((size_t)R.C, 1);
            if (R.out_buf < 2) std::printf("layer %d %d %d\n", R.C, R.Ho, R.Wo);
        }
    }
    CHECK(convs == CNN_NUM_CONVS && pools == CNN_NUM_POOLS && blob_at == P.blob_floats);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // what is refused, and the smallest side
    CHECK(cnn_min_side() == 15);
    CHECK(!cnn_make_plan(0, 224, 224, CNN_IN_F32_NCHW).ok && !cnn_make_plan(1, 14, 224, CNN_IN_F32_NCHW).ok);
    CHECK(!cnn_make_plan(1, 224, 14, CNN_IN_U8_NHWC).ok && !cnn_make_plan(1, 224, 224, CNN_IN_F32_NHWC).ok);
    CHECK(cnn_make_plan(1, 15, 17, CNN_IN_F32_NCHW).ok && cnn_make_plan(1, 15, 15, CNN_IN_U8_NHWC).ok);
    CHECK(!cnn_make_plan(1 << 20, 224, 224, CNN_IN_F32_NCHW).ok);                    // rows past 2^30
    CHECK(cnn_pool_out(7, 3, 2, 0, 1) == 3 && cnn_pool_out(8, 3, 2, 0, 1) == 4 && cnn_pool_out(1, 2, 2, 0, 1) == 1);
    CHECK(cnn_pool_out(2, 3, 2, 0, 1) == 1 && cnn_pool_out(1, 3, 2, 0, 1) == 0 && cnn_pool_out(5, 3, 1, 1, 1) == 5);
    for (int i = 1; i + 2 < argc; i += 3) {
        const int N = std::atoi(argv[i]), H = std::atoi(argv[i + 1]), W = std::atoi(argv[i + 2]);
        for (int layout : {CNN_IN_F32_NCHW, CNN_IN_U8_NHWC}) {
            std::printf("shape %d %d %d %d\n", N, H, W, layout);
            if (walk(N, H, W, layout)) return 1;
        }
    }
    std::printf("OK\n");
    return 0;
}
