// csrc/vs_cnn3d_plan.h alone, as plain C++17 (no HIP): tests/test_cnn3d_plan_host.py builds this with the host compiler and
// -fsanitize=address,undefined and runs it as a program.  For each (N, T, H, W) on the command line and both input kinds it makes
// the plan and walks every record with the functions the kernel itself calls (cnn3d_pos / cnn3d_tap / cnn3d_offset /
// cnn3d_store_offset), over the whole padded tile grid:
//   - every non-negative input offset is inside the input; padding taps, k >= K and rows >= M read nothing;
//   - a 16-byte load (every layer but the stem) is 16-byte aligned and stays inside one tap;
//   - every output element's store offset is inside its buffer and is hit exactly once; guard rows and columns store nothing;
//   - a record's source, residual and destination buffers never alias, and each buffer read holds the tensor the record expects;
//   - the packed-weight offsets tile the blob without overlap.
// It prints one line per record, "conv <cout> <to> <ho> <wo>", for the test to compare with torch's own sizes, then "OK".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vs_cnn3d_plan.h"

#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAILED line %d: %s\n", __LINE__, #__VA_ARGS__); return 1; } } while (0)

namespace {

struct Tensor { int64_t n = 0, t = 0, h = 0, w = 0, c = 0; };      // what a workspace buffer holds

int walk(int32_t N, int32_t T, int32_t H, int32_t W, int32_t layout) {
    const Cnn3dPlan P = cnn3d_make_plan(N, T, H, W, layout);
    CHECK(P.ok);
    for (int b = 0; b < CNN3D_NUM_BUFS; ++b) {                      // the buffers: in order, disjoint, 256-byte aligned, inside the workspace
        CHECK(P.buf_off[b] % 64 == 0 && P.buf_floats[b] > 0);
        const int64_t end = P.buf_off[b] + P.buf_floats[b];
        CHECK(end <= (b + 1 < CNN3D_NUM_BUFS ? P.buf_off[b + 1] : P.workspace_bytes / 4));
    }
    Tensor held[CNN3D_NUM_BUFS];
    int64_t blob_at = 0, flops = 0;
    for (int i = 0; i < CNN3D_NUM_CONVS; ++i) {
        const Cnn3dConvRec &R = P.conv[i];
        const Cnn3dConv &g = R.g;
        CHECK(g.N == N && g.K == g.kt * g.ks * g.ks * g.Cin && g.Kp % CNN3D_TILE_K == 0 && g.Kp >= g.K && g.Kp - g.K < CNN3D_TILE_K);
        CHECK(g.Coutp % CNN3D_TILE_N == 0 && g.Coutp >= g.Cout && g.Coutp - g.Cout < CNN3D_TILE_N);
        CHECK(g.To >= 1 && g.Ho >= 1 && g.Wo >= 1 && g.M == (int64_t)N * g.To * g.Ho * g.Wo);
        CHECK(R.w_off == blob_at && R.b_off == R.w_off + (int64_t)g.Coutp * g.Kp);       // the blob: tiled without gap or overlap
        blob_at = R.b_off + g.Coutp;
        flops += cnn3d_flops(g);
        // source, residual, destination: distinct buffers, and what is read is what was written there last
        CHECK(R.out_buf >= 0 && R.out_buf < CNN3D_NUM_BUFS && R.in_buf != R.out_buf && R.res_buf != R.out_buf);
        int64_t in_elems;
        bool vec4;
        if (R.in_buf == CNN3D_BUF_INPUT) {
            CHECK(i == 0 && g.Cin == 3 && g.T == T && g.H == H && g.W == W && R.res_buf == CNN3D_BUF_NONE && R.relu == 1);
            in_elems = (int64_t)N * 3 * T * H * W;
            vec4 = false;
        } else {
            CHECK(R.in_buf >= 0 && R.in_buf < CNN3D_NUM_BUFS);
            const Tensor &S = held[R.in_buf];
            CHECK(S.n == N && S.t == g.T && S.h == g.H && S.w == g.W && S.c == g.Cin);
            in_elems = (int64_t)N * g.T * g.H * g.W * g.Cin;
            CHECK(in_elems <= P.buf_floats[R.in_buf]);
            vec4 = true;
            CHECK(g.Cin % 4 == 0 && g.sc == 1 && g.sw == g.Cin && P.buf_off[R.in_buf] % 4 == 0);
        }
        if (R.res_buf != CNN3D_BUF_NONE) {
            CHECK(R.res_buf >= 0 && R.res_buf < CNN3D_NUM_BUFS && R.res_buf != R.in_buf && R.relu == 1);
            const Tensor &S = held[R.res_buf];
            CHECK(S.n == N && S.t == g.To && S.h == g.Ho && S.w == g.Wo && S.c == g.Cout);   // the output's shape
        }
        // the gather over the padded rows of the tile grid: first and last load of every tap, and the k padding
        const int64_t Mp = (g.M + CNN3D_TILE_M - 1) / CNN3D_TILE_M * CNN3D_TILE_M;
        const int span = vec4 ? 4 : 1, taps = g.kt * g.ks * g.ks;
        for (int64_t m = 0; m < Mp; ++m) {
            const Cnn3dPos px = cnn3d_pos(g, m);
            CHECK(px.valid == (m < g.M));
            int64_t n_inside = 0;
            for (int tap = 0; tap < taps; ++tap) {
                const int ks[2] = {tap * g.Cin, tap * g.Cin + g.Cin - span};
                for (int k : ks) {
                    const Cnn3dTap tp = cnn3d_tap(g, k);
                    CHECK(tp.valid && tp.dt == tap / (g.ks * g.ks) && tp.dh == tap / g.ks % g.ks && tp.dw == tap % g.ks && tp.c == k - tap * g.Cin);
                    if (vec4) {                                     // the 4 floats of a 16-byte load lie in one tap
                        const Cnn3dTap last = cnn3d_tap(g, k + 3);
                        CHECK(k % 4 == 0 && last.valid && last.dt == tp.dt && last.dh == tp.dh && last.dw == tp.dw && last.c == tp.c + 3);
                    }
                    const int64_t off = cnn3d_offset(g, px, tp);
                    const int ti = px.ti0 + tp.dt, hi = px.hi0 + tp.dh, wi = px.wi0 + tp.dw;
                    const bool inside = px.valid && ti >= 0 && ti < g.T && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
                    CHECK((off >= 0) == inside);
                    if (inside) {
                        CHECK(off + span <= in_elems);
                        if (vec4) CHECK(off % 4 == 0);
                        ++n_inside;
                    }
                }
            }
            if (px.valid) CHECK(n_inside > 0);                     // every output position sees the input
            for (int k = g.K; k < g.Kp; ++k) CHECK(cnn3d_offset(g, px, cnn3d_tap(g, k)) == -1);
        }
        CHECK(!cnn3d_tap(g, -1).valid && !cnn3d_pos(g, -1).valid);
        // the stores over the whole padded tile grid: inside the buffer, each element exactly once, nothing from a guard
        std::vector<unsigned char> hit((size_t)(g.M * g.Cout), 0);
        CHECK(g.M * g.Cout <= P.buf_floats[R.out_buf]);
        for (int64_t m = 0; m < Mp; ++m)
            for (int col = 0; col < g.Coutp; ++col) {
                const int64_t off = cnn3d_store_offset(g, m, col);
                CHECK((off >= 0) == (m < g.M && col < g.Cout));
                if (off < 0) continue;
                CHECK(off < g.M * g.Cout && !hit[(size_t)off]);
                hit[(size_t)off] = 1;
            }
        for (unsigned char x : hit) CHECK(x);
        held[R.out_buf] = Tensor{N, g.To, g.Ho, g.Wo, g.Cout};
        std::printf("conv %d %d %d %d\n", g.Cout, g.To, g.Ho, g.Wo);
    }
    CHECK(blob_at == P.blob_floats && flops == P.flops);
    const Tensor &L = held[P.pool_buf];
    CHECK(L.c == CNN3D_FEATURES && L.n == N && P.pool_positions == L.t * L.h * L.w && P.pool_positions >= 1);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // what is refused; every size from 1 is accepted
    CHECK(!cnn3d_make_plan(0, 16, 112, 112, CNN3D_IN_F32_NCDHW).ok && !cnn3d_make_plan(1, 0, 112, 112, CNN3D_IN_F32_NCDHW).ok);
    CHECK(!cnn3d_make_plan(1, 16, 0, 112, CNN3D_IN_U8_NDHWC).ok && !cnn3d_make_plan(1, 16, 112, 0, CNN3D_IN_U8_NDHWC).ok);
    CHECK(!cnn3d_make_plan(1, 16, 112, 112, CNN3D_IN_F32_NDHWC).ok);
    CHECK(!cnn3d_make_plan(1 << 10, 1 << 10, 64, 64, CNN3D_IN_F32_NCDHW).ok);                // rows past 2^30
    CHECK(cnn3d_make_plan(1, 1, 1, 1, CNN3D_IN_U8_NDHWC).ok && cnn3d_make_plan(1, 1, 2, 3, CNN3D_IN_F32_NCDHW).ok);
    CHECK(cnn3d_conv_out(1, 3, 2, 1) == 1 && cnn3d_conv_out(2, 3, 2, 1) == 1 && cnn3d_conv_out(3, 3, 2, 1) == 2 && cnn3d_conv_out(1, 7, 2, 3) == 1);
    CHECK(cnn3d_conv_out(5, 1, 2, 0) == 3 && cnn3d_conv_out(2, 3, 1, 0) == 0);
    for (int i = 1; i + 3 < argc; i += 4) {
        const int N = std::atoi(argv[i]), T = std::atoi(argv[i + 1]), H = std::atoi(argv[i + 2]), W = std::atoi(argv[i + 3]);
        for (int layout : {CNN3D_IN_F32_NCDHW, CNN3D_IN_U8_NDHWC}) {
            std::printf("shape %d %d %d %d %d\n", N, T, H, W, layout);
            if (walk(N, T, H, W, layout)) return 1;
        }
    }
    std::printf("OK\n");
    return 0;
}
