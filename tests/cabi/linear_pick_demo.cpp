// csrc/vs_linear_pick.h alone, as plain C++17 (no HIP): tests/test_linear_pick_host.py builds this with the host compiler and
// -fsanitize=address,undefined.  Part 1: named cases -> the expected pick, written out by hand from the branch structure the
// launchers had before the pick existed (every family and every template tuple is reached); part 2: the refusals; part 3: over
// a grid the pick is total, only names instantiations that exist, names every one that exists, and its geometry covers the
// output without overflow.  Prints "OK" or the first failed check.
#include <cstdio>
#include <set>
#include <tuple>

#include "vs_linear_pick.h"

#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAILED line %d: %s\n", __LINE__, #__VA_ARGS__); return 1; } } while (0)

namespace {

// the mode words in use (vs_forward_plan.h, vs_train_plan.h, the per-op C entries)
const int X = 0, B16 = 1, H3 = 2, S16 = 1 | VSK_STORE16, A16 = 1 | VSK_A16, F16 = 1 | VSK_F16, SF16 = S16 | VSK_F16, AF16 = A16 | VSK_F16;
const int STORE = VSK_STORE16, ABIT = VSK_A16, FBIT = VSK_F16;      // the bare bits: no mode without 16-bit operands
const int WORDS[] = {X, B16, H3, S16, A16, F16, SF16, AF16};
const int SR = 16384;                      // VS_SKINNY_ROWS default; 0 switches the latency kernels off
const size_t LDS_K256 = 32 * (256 + 4) * 4, LDS_K1024 = 32 * (1024 + 4) * 4;

const VskGemmFamily SK2 = VSK_GEMM_SKINNY2, SK1 = VSK_GEMM_SKINNY, TIL = VSK_GEMM_TILED;

struct GemmCase {
    const char *name;
    int epi, M, N, K, word;
    bool wf;
    int sr;
    VskGemmFamily family;
    int nwm, nj, prec, c16, kw, a16;       // TILED
    int gx, gy;                            // skinny families
    size_t lds;
    int ntiles, per_cu;                    // TILED
};

const GemmCase GEMM_CASES[] = {
    // ---- exact fp32 ----
    {"exact, latency kernels off: 128x128 tiles", EPI_BIAS, 100, 256, 256, X, false, 0, TIL, 2, 2, 0, 0, 32, 0, 0, 0, 0, 2, 2},
    {"exact, no weight copy, M <= skinny_rows: first-generation skinny", EPI_BIAS, 100, 256, 256, X, false, SR, SK1, 0, 0, 0, 0, 0, 0, 4, 2, 0, 0, 0},
    {"exact, weight copy, M <= skinny_rows: skinny2", EPI_RELU, 100, 1024, 256, X, true, SR, SK2, 0, 0, 0, 0, 0, 0, 4, 8, LDS_K256, 0, 0},
    {"exact skinny2, K = 2048: LDS of 1024 k", EPI_BIAS, 100, 256, 2048, X, true, SR, SK2, 0, 0, 0, 0, 0, 0, 4, 2, LDS_K1024, 0, 0},
    {"M = skinny_rows is the last skinny row count", EPI_QKV, 16384, 768, 256, X, true, SR, SK2, 0, 0, 0, 0, 0, 0, 512, 6, LDS_K256, 0, 0},
    {"M = skinny_rows + 1 is tiled (390 wide tiles: 128x128)", EPI_QKV, 16385, 768, 256, X, true, SR, TIL, 2, 2, 0, 0, 32, 0, 0, 0, 0, 129 * 6, 2},
    {"K % 128 != 0 is tiled", EPI_BIAS, 100, 256, 192, X, true, SR, TIL, 2, 2, 0, 0, 32, 0, 0, 0, 0, 2, 2},
    {"N % 32 != 0 is tiled", EPI_BIAS, 100, 48, 256, X, false, SR, TIL, 2, 2, 0, 0, 32, 0, 0, 0, 0, 1, 2},
    {"(16128, 1024): 504 wide tiles, one row of tiles short", EPI_RELU, 16128, 1024, 256, X, false, 0, TIL, 2, 2, 0, 0, 32, 0, 0, 0, 0, 126 * 8, 2},
    {"(16129, 1024): the first M with 512 wide tiles", EPI_RELU, 16129, 1024, 256, X, false, 0, TIL, 4, 4, 0, 0, 32, 0, 0, 0, 0, 64 * 4, 1},
    {"(16384, 1024): 512 wide tiles, no ragged edge", EPI_RELU, 16384, 1024, 256, X, false, 0, TIL, 4, 4, 0, 0, 32, 0, 0, 0, 0, 64 * 4, 1},
    {"(16385, 1024) above skinny_rows", EPI_RELU, 16385, 1024, 256, X, true, SR, TIL, 4, 4, 0, 0, 32, 0, 0, 0, 0, 65 * 4, 1},
    {"wide, N = 384 (N % 256 != 0): 256x128 tiles", EPI_PE, 43776, 384, 256, X, false, SR, TIL, 4, 2, 0, 0, 32, 0, 0, 0, 0, 171 * 3, 1},
    {"520 wide tiles but r256 * 100 > r128 * 105: 128x128 tiles", EPI_BIAS, 2400, 6656, 256, X, false, 0, TIL, 2, 2, 0, 0, 32, 0, 0, 0, 0, 19 * 52, 2},
    {"the same N with r256 == r128", EPI_BIAS, 2433, 6656, 256, X, false, 0, TIL, 4, 4, 0, 0, 32, 0, 0, 0, 0, 10 * 26, 1},
    {"exact GATE, tiled", EPI_GATE, 140, 1024, 256, X, false, 0, TIL, 2, 2, 0, 0, 32, 0, 0, 0, 0, 2 * 8, 2},
    {"exact RELU_DROP, skinny2", EPI_RELU_DROP, 140, 1024, 256, X, true, SR, SK2, 0, 0, 0, 0, 0, 0, 5, 8, LDS_K256, 0, 0},
    // ---- fp16x3 ----
    {"fp16x3, weight copy, M <= skinny_rows: skinny2<., 2>", EPI_PE, 100, 256, 1024, H3, true, SR, SK2, 0, 0, 2, 0, 0, 0, 4, 2, LDS_K1024, 0, 0},
    {"fp16x3 without its weight copy is tiled at every M", EPI_BIAS, 100, 256, 256, H3, false, SR, TIL, 2, 2, 2, 0, 32, 0, 0, 0, 0, 2, 2},
    {"fp16x3 M = 128: 128x128 tiles", EPI_BIAS, 128, 256, 256, H3, false, 0, TIL, 2, 2, 2, 0, 32, 0, 0, 0, 0, 2, 2},
    {"fp16x3 M = 129: 256x256 tiles", EPI_BIAS, 129, 256, 256, H3, false, 0, TIL, 4, 4, 2, 0, 32, 0, 0, 0, 0, 1, 1},
    {"fp16x3 K = 512: no 64-wide k-tiles", EPI_RELU, 129, 1024, 512, H3, true, 0, TIL, 4, 4, 2, 0, 32, 0, 0, 0, 0, 4, 1},
    // ---- bf16 / f16 operands, fp32 storage ----
    {"bf16 at M <= skinny_rows with a weight copy is still tiled", EPI_BIAS, 100, 256, 256, B16, true, SR, TIL, 2, 2, 1, 0, 32, 0, 0, 0, 0, 2, 2},
    {"bf16 M = 128, K = 512", EPI_BIAS, 128, 256, 512, B16, false, SR, TIL, 2, 2, 1, 0, 64, 0, 0, 0, 0, 2, 2},
    {"bf16 M = 129, K = 512", EPI_BIAS, 129, 256, 512, B16, false, SR, TIL, 4, 4, 1, 0, 64, 0, 0, 0, 0, 1, 1},
    {"bf16 M = 129, K = 448: K % 64 == 0 but below 512", EPI_BIAS, 129, 256, 448, B16, false, SR, TIL, 4, 4, 1, 0, 32, 0, 0, 0, 0, 1, 1},
    {"bf16 M = 128, K = 256", EPI_PE, 128, 256, 256, B16, false, SR, TIL, 2, 2, 1, 0, 32, 0, 0, 0, 0, 2, 2},
    {"bf16 N = 384: N % 256 != 0 keeps 128x128 tiles", EPI_BIAS, 129, 384, 512, B16, false, SR, TIL, 2, 2, 1, 0, 64, 0, 0, 0, 0, 2 * 3, 2},
    {"f16 M = 129, K = 512", EPI_QKV, 129, 768, 512, F16, false, SR, TIL, 4, 4, 3, 0, 64, 0, 0, 0, 0, 3, 1},
    {"f16 M = 129, K = 256", EPI_GATE, 129, 1024, 256, F16, false, SR, TIL, 4, 4, 3, 0, 32, 0, 0, 0, 0, 4, 1},
    {"f16 M = 128, K = 512", EPI_RELU_DROP, 128, 1024, 512, F16, false, SR, TIL, 2, 2, 3, 0, 64, 0, 0, 0, 0, 8, 2},
    {"f16 M = 128, K = 256", EPI_RELU, 128, 1024, 256, F16, true, SR, TIL, 2, 2, 3, 0, 32, 0, 0, 0, 0, 8, 2},
    // ---- 16-bit C ----
    {"STORE16 BIAS, 128x128 tiles, K = 512: 32-wide k-tiles", EPI_BIAS, 128, 256, 512, S16, false, SR, TIL, 2, 2, 1, 1, 32, 0, 0, 0, 0, 2, 2},
    {"STORE16 RELU, the same shape: 64-wide k-tiles", EPI_RELU, 128, 256, 512, S16, false, SR, TIL, 2, 2, 1, 1, 64, 0, 0, 0, 0, 2, 2},
    {"STORE16 GATE, 128x128 tiles, K = 512", EPI_GATE, 100, 1024, 512, S16, false, SR, TIL, 2, 2, 1, 1, 32, 0, 0, 0, 0, 8, 2},
    {"STORE16 RELU_DROP, 128x128 tiles, K = 512", EPI_RELU_DROP, 100, 1024, 512, S16, false, SR, TIL, 2, 2, 1, 1, 32, 0, 0, 0, 0, 8, 2},
    {"STORE16 QKV, 128x128 tiles, K = 512", EPI_QKV, 128, 768, 512, S16, false, SR, TIL, 2, 2, 1, 1, 64, 0, 0, 0, 0, 6, 2},
    {"STORE16 RELU, 128x128 tiles, K = 256", EPI_RELU, 128, 1024, 256, S16, false, SR, TIL, 2, 2, 1, 1, 32, 0, 0, 0, 0, 8, 2},
    {"STORE16 QKV, 128x128 tiles, K = 448", EPI_QKV, 128, 768, 448, S16, false, SR, TIL, 2, 2, 1, 1, 32, 0, 0, 0, 0, 6, 2},
    {"STORE16 RELU, 256x256 tiles, K = 512", EPI_RELU, 129, 1024, 512, S16, false, SR, TIL, 4, 4, 1, 1, 64, 0, 0, 0, 0, 4, 1},
    {"STORE16 QKV, 256x256 tiles, K = 512", EPI_QKV, 129, 1536, 512, S16, true, SR, TIL, 4, 4, 1, 1, 64, 0, 0, 0, 0, 6, 1},
    {"STORE16 BIAS, 256x256 tiles, K = 512", EPI_BIAS, 129, 256, 512, S16, false, SR, TIL, 4, 4, 1, 1, 64, 0, 0, 0, 0, 1, 1},
    {"STORE16 GATE, 256x256 tiles, K = 256", EPI_GATE, 129, 256, 256, S16, false, SR, TIL, 4, 4, 1, 1, 32, 0, 0, 0, 0, 1, 1},
    {"STORE16 QKV, 256x256 tiles, K = 256", EPI_QKV, 140, 768, 256, S16, true, SR, TIL, 4, 4, 1, 1, 32, 0, 0, 0, 0, 3, 1},
    {"STORE16 | F16 RELU_DROP, 256x256 tiles, K = 256", EPI_RELU_DROP, 140, 1024, 256, SF16, false, SR, TIL, 4, 4, 3, 1, 32, 0, 0, 0, 0, 4, 1},
    {"STORE16 | F16 RELU_DROP, 256x256 tiles, K = 512", EPI_RELU_DROP, 140, 2048, 512, SF16, false, SR, TIL, 4, 4, 3, 1, 64, 0, 0, 0, 0, 8, 1},
    {"STORE16 | F16 RELU_DROP, 128x128 tiles", EPI_RELU_DROP, 70, 1024, 256, SF16, false, SR, TIL, 2, 2, 3, 1, 32, 0, 0, 0, 0, 8, 2},
    {"STORE16 | F16 RELU, 128x128 tiles, K = 512", EPI_RELU, 70, 2048, 512, SF16, false, SR, TIL, 2, 2, 3, 1, 64, 0, 0, 0, 0, 16, 2},
    // ---- 16-bit A ----
    {"A16 BIAS, 128x128 tiles, K = 512: 32-wide k-tiles", EPI_BIAS, 128, 256, 512, A16, false, SR, TIL, 2, 2, 1, 0, 32, 1, 0, 0, 0, 2, 2},
    {"A16 PE, 256x256 tiles, K = 512", EPI_PE, 129, 256, 512, A16, false, SR, TIL, 4, 4, 1, 0, 64, 1, 0, 0, 0, 1, 1},
    {"A16 BIAS, 256x256 tiles, K = 256", EPI_BIAS, 129, 256, 256, A16, false, SR, TIL, 4, 4, 1, 0, 32, 1, 0, 0, 0, 1, 1},
    {"A16 | F16 BIAS, 256x256 tiles, K = 1024", EPI_BIAS, 140, 256, 1024, AF16, true, SR, TIL, 4, 4, 3, 0, 64, 1, 0, 0, 0, 1, 1},
    {"A16 | F16 PE, 256x256 tiles, K = 256", EPI_PE, 140, 256, 256, AF16, false, SR, TIL, 4, 4, 3, 0, 32, 1, 0, 0, 0, 1, 1},
    {"A16 | F16 BIAS, 128x128 tiles, K = 1024", EPI_BIAS, 70, 256, 1024, AF16, false, SR, TIL, 2, 2, 3, 0, 32, 1, 0, 0, 0, 2, 2},
};

const VskLnFamily LSK2 = VSK_LN_SKINNY2, LSK1 = VSK_LN_SKINNY, LROWS = VSK_LN_ROWS, LRES = VSK_LN_RES;

struct LnCase {
    const char *name;
    int M, N, K, word;
    bool wf;
    int sr;
    VskLnFamily family;
    int width, prec, a16, grid, block;
    size_t lds;
};

const LnCase LN_CASES[] = {
    {"fp16x3, weight copy, M <= skinny_rows: skinny2_ln<8, 2>", 100, 256, 256, H3, true, SR, LSK2, 8, 2, 0, 4, 512, LDS_K256},
    {"fp16x3 without its copy: gemm_ln_rows<8, 2>", 100, 256, 256, H3, false, SR, LROWS, 8, 2, 0, 0, 256, 0},
    {"bf16, A stored as bf16: gemm_ln_rows<8, 1, 1>", 300, 256, 1024, S16, true, SR, LROWS, 8, 1, 1, 0, 256, 0},
    {"bf16: gemm_ln_rows<2, 1>", 300, 64, 256, B16, true, SR, LROWS, 2, 1, 0, 0, 256, 0},
    {"exact, weight copy: skinny2_ln<4, 0>", 100, 128, 1024, X, true, SR, LSK2, 4, 0, 0, 4, 256, LDS_K1024},
    {"exact, no copy: skinny_ln<6>", 100, 192, 256, X, false, SR, LSK1, 6, 0, 0, 4, 384, 0},
    {"exact, M = skinny_rows", 16384, 256, 256, X, true, SR, LSK2, 8, 0, 0, 512, 512, LDS_K256},
    {"exact, M = skinny_rows + 1: gemm_ln_rows<8, 0>", 16385, 256, 256, X, true, SR, LROWS, 8, 0, 0, 0, 256, 0},
    {"exact, K % 128 != 0: gemm_ln_rows", 100, 256, 192, X, true, SR, LROWS, 8, 0, 0, 0, 256, 0},
    {"exact, latency kernels off", 100, 64, 256, X, false, 0, LROWS, 2, 0, 0, 0, 256, 0},
    {"exact, N = 512: gemm_res_ln<8, 0>", 100, 512, 256, X, true, SR, LRES, 8, 0, 0, 2, 256, 0},
    {"exact, N = 320: gemm_res_ln<5, 0>", 129, 320, 256, X, false, SR, LRES, 5, 0, 0, 3, 256, 0},
    {"fp16x3, N = 512: gemm_res_ln<8, 2>", 100, 512, 256, H3, true, SR, LRES, 8, 2, 0, 2, 256, 0},
};

typedef std::tuple<int, int, int, int, int, int> Tuple;       // nwm, nj, prec, c16, kw, a16
Tuple tuple_of(const VskGemmPick &p) { return Tuple(p.nwm, p.nj, p.prec, p.c16, p.kw, p.a16); }

bool same(const VskGemmPick &p, const GemmCase &c) {
    return p.family == c.family && p.prec == c.prec && p.nwm == c.nwm && p.nj == c.nj && p.c16 == c.c16 && p.kw == c.kw && p.a16 == c.a16 &&
           p.grid_x == c.gx && p.grid_y == c.gy && p.lds == c.lds && p.ntiles == c.ntiles && p.per_cu == c.per_cu;
}

int run() {
    // ---- the mode word ----
    std::set<int> valid(WORDS, WORDS + sizeof WORDS / sizeof *WORDS);
    for (int w = -2; w < 512; ++w) CHECK(vsk_linear_mode(w).valid == (valid.count(w) != 0));
    for (int w : WORDS) {
        const VskLinearMode m = vsk_linear_mode(w);
        CHECK(m.arith == (w & 3) && m.store16 == ((w & VSK_STORE16) != 0) && m.a16 == ((w & VSK_A16) != 0) && m.f16 == ((w & VSK_F16) != 0));
    }

    // ---- part 1: named cases ----
    std::set<int> families;
    std::set<Tuple> tuples;
    for (const GemmCase &c : GEMM_CASES) {
        const VskGemmPick p = vsk_gemm_pick(c.epi, c.M, c.N, c.K, c.word, c.wf, c.sr);
        if (!same(p, c)) {
            std::printf("FAILED gemm case '%s': family %d <%d, %d, %d, %d, %d, %d> grid %d x %d lds %zu ntiles %d per_cu %d\n", c.name, (int)p.family,
                        p.nwm, p.nj, p.prec, p.c16, p.kw, p.a16, p.grid_x, p.grid_y, p.lds, p.ntiles, p.per_cu);
            return 1;
        }
        families.insert(p.family * 10 + (p.family == TIL ? 0 : p.prec));
        if (p.family == TIL) tuples.insert(tuple_of(p));
    }
    // both skinny generations in both precisions, and every template tuple any epilogue has
    CHECK(families == std::set<int>({SK2 * 10, SK2 * 10 + 2, SK1 * 10, TIL * 10}));
    std::set<Tuple> all_tuples;
    for (int epi = 0; epi < EPI_COUNT; ++epi)
        for (int nwm = 1; nwm <= 5; ++nwm) for (int nj = 1; nj <= 5; ++nj) for (int prec = -1; prec <= 4; ++prec)
            for (int c16 = 0; c16 <= 1; ++c16) for (int kw = 16; kw <= 128; kw *= 2) for (int a16 = 0; a16 <= 1; ++a16)
                if (vsk_gemm_tuple_legal(epi, nwm, nj, prec, c16, kw, a16)) all_tuples.insert(Tuple(nwm, nj, prec, c16, kw, a16));
    CHECK(all_tuples.size() == 27);
    CHECK(tuples == all_tuples);

    std::set<int> ln_forms;
    for (const LnCase &c : LN_CASES) {
        const VskLnPick p = vsk_ln_pick(c.M, c.N, c.K, c.word, c.wf, c.sr);
        if (!(p.family == c.family && p.width == c.width && p.prec == c.prec && p.a16 == c.a16 && p.grid == c.grid && p.block == c.block &&
              p.lds == c.lds)) {
            std::printf("FAILED ln case '%s': family %d width %d prec %d a16 %d grid %d block %d lds %zu\n", c.name, (int)p.family, p.width, p.prec,
                        p.a16, p.grid, p.block, p.lds);
            return 1;
        }
        ln_forms.insert(p.family * 100 + p.prec * 10 + p.a16);
    }
    // the seven launch branches: skinny2_ln<., 2 | 0>, skinny_ln, gemm_ln_rows<., 2 | 1 + A16 | 1 | 0>, gemm_res_ln<., 2 | 0>
    CHECK(ln_forms == std::set<int>({LSK2 * 100 + 20, LSK2 * 100, LSK1 * 100, LROWS * 100 + 20, LROWS * 100 + 11, LROWS * 100 + 10, LROWS * 100,
                                     LRES * 100 + 20, LRES * 100}));

    // ---- shared helpers ----
    CHECK(vsk_head_dim_shift(32) == 5 && vsk_head_dim_shift(64) == 6 && vsk_head_dim_shift(128) == 7 && vsk_head_dim_shift(256) == 8);
    CHECK(vsk_skinny2_lds(128) == 32 * 132 * 4 && vsk_skinny2_lds(4096) == LDS_K1024);
    CHECK(vsk_persistent_blocks(1, 2, 256) == 8 && vsk_persistent_blocks(1000, 2, 256) == 512 && vsk_persistent_blocks(1000, 1, 256) == 256);
    CHECK(vsk_persistent_blocks(1000, 2, 304) == 608 && vsk_persistent_blocks(1000, 1, 1) == 8 && vsk_persistent_blocks(100, 2, 256) == 104);
    CHECK(vsk_row_tile_grid(100, 256) == 1 && vsk_row_tile_grid(300, 256) == 3 && vsk_row_tile_grid(1 << 20, 256) == 512);

    // ---- part 2: refusals ----
    for (int epi : {EPI_RELU, EPI_QKV, EPI_GATE, EPI_RELU_DROP})
        for (int w : {A16, AF16}) CHECK(vsk_gemm_pick(epi, 300, 256, 512, w, false, SR).family == VSK_GEMM_UNSUPPORTED);
    for (int w : {S16, SF16}) CHECK(vsk_gemm_pick(EPI_PE, 300, 256, 512, w, false, SR).family == VSK_GEMM_UNSUPPORTED);
    for (int epi = 0; epi < EPI_COUNT; ++epi) {
        // STORE16 | A16 together; the storage bits or F16 without 16-bit operands; words that are no mode
        for (int w : {S16 | ABIT, SF16 | ABIT, STORE, ABIT, FBIT, H3 | STORE, H3 | ABIT, H3 | FBIT, 3, 8, 128 | 1, -1})
            CHECK(vsk_gemm_pick(epi, 300, 256, 512, w, true, SR).family == VSK_GEMM_UNSUPPORTED);
    }
    CHECK(vsk_gemm_pick(EPI_COUNT, 300, 256, 512, X, true, SR).family == VSK_GEMM_UNSUPPORTED);
    CHECK(vsk_gemm_pick(-1, 300, 256, 512, X, true, SR).family == VSK_GEMM_UNSUPPORTED);
    for (int w : {B16, S16}) {                 // bf16 Linear + LayerNorm: N <= 256, a multiple of 32
        CHECK(vsk_ln_pick(300, 512, 256, w, true, SR).family == VSK_LN_UNSUPPORTED);
        CHECK(vsk_ln_pick(300, 320, 256, w, true, SR).family == VSK_LN_UNSUPPORTED);
        CHECK(vsk_ln_pick(300, 80, 256, w, true, SR).family == VSK_LN_UNSUPPORTED);
    }
    CHECK(vsk_ln_pick(300, 80, 256, H3, true, SR).family == VSK_LN_UNSUPPORTED);
    for (int w : {X, B16, H3, S16})            // N / 32 is 2, 4, 6 or 8
        for (int N : {32, 96, 160, 224}) CHECK(vsk_ln_pick(300, N, 256, w, true, SR).family == VSK_LN_UNSUPPORTED);
    for (int w : {X, H3})                      // N / 64 outside 1 .. 8
        for (int N : {576, 640, 1024}) CHECK(vsk_ln_pick(300, N, 256, w, true, SR).family == VSK_LN_UNSUPPORTED);
    CHECK(vsk_ln_pick(300, 16, 256, X, true, SR).family == VSK_LN_UNSUPPORTED);
    for (int w : {A16, F16, SF16, AF16, S16 | ABIT, H3 | STORE, STORE, 3, -1})
        CHECK(vsk_ln_pick(300, 256, 256, w, true, SR).family == VSK_LN_UNSUPPORTED);

    // ---- part 3: a grid ----
    const int MS[] = {1, 31, 32, 33, 100, 128, 129, 255, 256, 257, 1000, 16128, 16129, 16384, 16385, 43776, 65537, 1 << 20};
    const int NS[] = {32, 48, 64, 96, 128, 192, 256, 320, 384, 512, 768, 1024, 2048, 6656};
    const int KS[] = {32, 64, 128, 192, 256, 448, 512, 1024, 2048};
    const int CUS[] = {1, 8, 256, 304};
    std::set<std::pair<int, Tuple>> reached;
    for (int M : MS) for (int N : NS) for (int K : KS) for (int w : WORDS) for (int wf = 0; wf <= 1; ++wf) for (int sr : {0, SR}) {
        const VskLinearMode m = vsk_linear_mode(w);
        for (int epi = 0; epi < EPI_COUNT; ++epi) {
            const VskGemmPick p = vsk_gemm_pick(epi, M, N, K, w, wf != 0, sr);
            const bool refused = (m.a16 && epi != EPI_BIAS && epi != EPI_PE) || (m.store16 && epi == EPI_PE);
            CHECK((p.family == VSK_GEMM_UNSUPPORTED) == refused);
            if (refused) continue;
            if (p.family == TIL) {
                CHECK(vsk_gemm_tuple_legal(epi, p.nwm, p.nj, p.prec, p.c16, p.kw, p.a16));
                CHECK(p.prec == (m.arith == 1 ? (m.f16 ? 3 : 1) : m.arith) && p.c16 == (int)m.store16 && p.a16 == (int)m.a16);
                // 64-wide k-tiles exactly where K allows them and that instantiation exists
                CHECK((p.kw == 64) == (m.arith == 1 && K % 64 == 0 && K >= 512 && vsk_gemm_tuple_legal(epi, p.nwm, p.nj, p.prec, p.c16, 64, p.a16)));
                const long long bm = 64 * p.nwm, bn = 64 * p.nj, ntiles = ((M + bm - 1) / bm) * ((N + bn - 1) / bn);
                CHECK(ntiles > 0 && ntiles < (1ll << 31) && p.ntiles == ntiles);
                CHECK(p.per_cu == (p.nwm == 4 ? 1 : 2) && p.grid_x == 0 && p.grid_y == 0 && p.lds == 0);
                for (int cus : CUS) {
                    const int blocks = vsk_persistent_blocks(p.ntiles, p.per_cu, cus), cap = p.per_cu * cus / 8 * 8;
                    CHECK(blocks % 8 == 0 && blocks >= 8 && blocks <= (cap > 8 ? cap : 8) && blocks <= (p.ntiles + 7) / 8 * 8);
                }
                reached.insert(std::make_pair(epi, tuple_of(p)));
            } else {
                // the latency kernels: exact fp32 and fp16x3 only, M <= skinny_rows; the second generation iff the weight copy exists
                CHECK(m.arith != 1 && M <= sr && N % 32 == 0 && K % 128 == 0);
                CHECK((p.family == SK2) == (wf != 0) && p.prec == m.arith && (p.family == SK2 || m.arith == 0));
                CHECK(p.grid_x > 0 && p.grid_y > 0 && p.grid_x * 32ll >= M && p.grid_y * 128ll >= N && p.grid_y <= 65535);
                CHECK(p.lds == (p.family == SK2 ? (size_t)32 * ((K < 1024 ? K : 1024) + 4) * 4 : 0) && p.lds <= 160 * 1024);
                CHECK(p.ntiles == 0 && p.per_cu == 0 && p.nwm == 0);
            }
        }
        const VskLnPick q = vsk_ln_pick(M, N, K, w, wf != 0, sr);
        if (q.family == VSK_LN_UNSUPPORTED) continue;
        CHECK(!m.a16 && !m.f16 && q.prec == m.arith && q.a16 == (q.family == LROWS && m.store16 ? 1 : 0));
        if (q.family == LRES) {
            CHECK(m.arith != 1 && !(N <= 256 && N % 32 == 0) && q.width == N / 64 && q.width >= 1 && q.width <= 8);
            CHECK(q.grid > 0 && q.grid * 64ll >= M && q.block == 256 && q.lds == 0);
            continue;
        }
        CHECK(N <= 256 && q.width * 32 == N && q.width >= 2 && q.width <= 8 && q.width % 2 == 0);
        if (q.family == LROWS) {
            CHECK(q.grid == 0 && q.block == 256 && q.lds == 0);
            for (int cus : CUS) {
                const int blocks = vsk_row_tile_grid(M, cus), tiles = (M + 127) / 128;
                CHECK(blocks >= 1 && blocks <= tiles && blocks <= vsk_persistent_blocks(tiles, 2, cus));
            }
        } else {
            CHECK(m.arith != 1 && M <= sr && K % 128 == 0 && (q.family == LSK2) == (wf != 0) && (q.family == LSK2 || m.arith == 0));
            CHECK(q.grid > 0 && q.grid * 32ll >= M && q.block == 64 * q.width);
            CHECK(q.lds == (q.family == LSK2 ? (size_t)32 * ((K < 1024 ? K : 1024) + 4) * 4 : 0));
        }
    }
    // every instantiation that exists is one some shape runs
    size_t legal = 0;
    for (int epi = 0; epi < EPI_COUNT; ++epi)
        for (const Tuple &t : all_tuples)
            if (vsk_gemm_tuple_legal(epi, std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t), std::get<4>(t), std::get<5>(t))) {
                ++legal;
                CHECK(reached.count(std::make_pair(epi, t)) == 1);
            }
    CHECK(legal == 124 && reached.size() == legal);
    return 0;
}

}  // namespace

int main() {
    if (run()) return 1;
    std::printf("OK\n");
    return 0;
}
