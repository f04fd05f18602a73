// vs_linear_pick.h - which instantiation of which Linear kernel a launcher of vs_kernels.hip starts: a pure
// function of the epilogue, the shape, the mode word, whether a fragment-major weight copy exists, and VS_SKINNY_ROWS.
// launch_gemm and vsk_linear_res_ln pick, then only read the pick.
// Host code, plain C++17, no HIP and no globals: tests/cabi/linear_pick_demo.cpp compiles this header alone.
#pragma once
#include <stddef.h>

#include "vs_forward_plan.h"      // VSK_STORE16 / VSK_A16 / VSK_F16, vsk_layer_fused_supported

// epilogues of gemm_nt_128 / skinny_gemm / skinny2_gemm
enum { EPI_BIAS = 0, EPI_RELU = 1, EPI_PE = 2, EPI_QKV = 3,
       // training path only (vs_train.cpp):
       EPI_GATE = 4,          // C = gate > 0 ? C * scale : 0, gate = `pe` [M,N]: ReLU + dropout backward riding in the dgrad GEMM
       EPI_RELU_DROP = 5,     // C = dropout(relu(C)): mlp.dropout riding in the fc1 GEMM (reference simnet.py:181)
       EPI_COUNT = 6 };

// ---- the mode word, decoded once ----
// 0 exact fp32; 1 operands rounded to ONE 16-bit plane (bf16; | VSK_F16: IEEE f16, the training path's fp16 mode); 2 fp16x3 (fp32
// emulated with f16 hi + lo halves).  On 1 only: | VSK_STORE16 - the tensor that is only ever consumed as a 16-bit matrix operand
// lives in HBM as 16-bit (C of a GEMM, A of vsk_linear_res_ln; the rounding moves from the consumer to the producer: same bits,
// half the bytes); | VSK_A16 - A of a GEMM is stored as 16-bit.  Not both.  Every other word is invalid.
struct VskLinearMode {
    bool valid;
    int arith;                  // 0 exact, 1 16-bit operands, 2 fp16x3
    bool store16, a16, f16;
};

inline VskLinearMode vsk_linear_mode(int word) {
    VskLinearMode m{};
    m.arith = word & 15;
    m.store16 = (word & VSK_STORE16) != 0;
    m.a16 = (word & VSK_A16) != 0;
    m.f16 = (word & VSK_F16) != 0;
    m.valid = word >= 0 && !(word & ~(15 | VSK_STORE16 | VSK_A16 | VSK_F16)) && m.arith <= 2 &&
              (m.arith == 1 || !(m.store16 || m.a16 || m.f16)) && !(m.store16 && m.a16);
    return m;
}

// ---- geometry shared by the launchers ----
// persistent grid: `per_cu` blocks per CU, a multiple of 8 so the XCD chunking is exact
inline int vsk_persistent_blocks(int ntiles, int per_cu, int cus) {
    int g = per_cu * cus;
    g -= g % 8;
    if (g < 8) g = 8;
    const int need = (ntiles + 7) / 8 * 8;
    return need < g ? need : g;
}

// the kernels that walk 128-row tiles (gemm_ln_rows and the fused layer kernels): two blocks per CU, never more than tiles
inline int vsk_row_tile_grid(int M, int cus) {
    const int tiles = (M + 127) / 128, blocks = vsk_persistent_blocks(tiles, 2, cus);
    return blocks < tiles ? blocks : tiles;
}

// log2 of the head dim (32, 64, 128 or 256) for the kernels that scatter q / k / v head-major
inline int vsk_head_dim_shift(int dh) { return dh <= 32 ? 5 : dh <= 64 ? 6 : dh <= 128 ? 7 : 8; }

// 256-row tiles on 8-wave blocks when there is enough work to give every CU >= 2 such tiles and the
// ragged M edge does not waste more than 128-row tiles would; else 128x128 tiles on 4-wave blocks
inline bool vsk_use_wide_tiles(int M, int N) {
    const long r256 = (M + 255) / 256 * 256, r128 = (M + 127) / 128 * 128;
    const long tiles = (r256 / 256) * ((N + 127) / 128);
    return r256 * 100 <= r128 * 105 && tiles >= 512;
}

// dynamic LDS of the packed skinny kernels: 32 activation rows x (min(K,1024) + 4) floats (up to 128.5 KiB)
inline size_t vsk_skinny2_lds(int K) { return (size_t)32 * ((K < 1024 ? K : 1024) + 4) * sizeof(float); }

// ---- C = A W^T + bias (+ epilogue): launch_gemm ----
enum VskGemmFamily {
    VSK_GEMM_UNSUPPORTED = 0,
    VSK_GEMM_SKINNY2,       // skinny2_gemm<EPI, PREC>: the latency kernel on the fragment-major weight copy, PREC 0 or 2
    VSK_GEMM_SKINNY,        // skinny_gemm<EPI>: the first-generation latency kernel (no weight copy; exact fp32)
    VSK_GEMM_TILED,         // gemm_nt_128<EPI, NWM, 0, NJ, PREC, C16, KW, A16> on a persistent grid
};

struct VskGemmPick {
    VskGemmFamily family;
    int prec;                       // 0 exact, 1 bf16, 2 fp16x3, 3 f16
    int nwm, nj, c16, kw, a16;      // TILED: the template arguments that vary
    int grid_x, grid_y;             // skinny families: 32 rows x 128 columns per block ...
    size_t lds;                     // ... and their dynamic LDS bytes
    int ntiles, per_cu;             // TILED: vsk_persistent_blocks(ntiles, per_cu, CUs) blocks of 128 * nwm threads
};

// The instantiations of gemm_nt_128 that exist.  launch_gemm compiles a launch for exactly these (`if constexpr`), and
// vsk_gemm_pick returns no other tuple.
constexpr bool vsk_gemm_tuple_legal(int epi, int nwm, int nj, int prec, int c16, int kw, int a16) {
    const bool big = nwm == 4 && nj == 4, small = nwm == 2 && nj == 2;
    if (epi < 0 || epi >= EPI_COUNT || (kw != 32 && kw != 64) || (c16 != 0 && c16 != 1) || (a16 != 0 && a16 != 1)) return false;
    if (prec == 0) return (big || small || (nwm == 4 && nj == 2)) && !c16 && !a16 && kw == 32;
    if (prec == 2) return (big || small) && !c16 && !a16 && kw == 32;
    if ((prec != 1 && prec != 3) || !(big || small) || (c16 && a16)) return false;
    // 16-bit A: the two consumers of a 16-bit-stored tensor; their 128x128-tile form has 32-wide k-tiles only
    if (a16) return (epi == EPI_BIAS || epi == EPI_PE) && (big || kw == 32);
    // 16-bit C: fc1 and QKV (scoring and training) in every form; the training path's other producers without the
    // 128x128-tile form on 64-wide k-tiles; the positional epilogue has none
    if (c16) return epi == EPI_RELU || epi == EPI_QKV || (epi != EPI_PE && (big || kw == 32));
    return true;
}

inline VskGemmPick vsk_gemm_pick(int epi, int M, int N, int K, int word, bool has_wf, int skinny_rows) {
    VskGemmPick p{};
    const VskLinearMode m = vsk_linear_mode(word);
    if (!m.valid || epi < 0 || epi >= EPI_COUNT) return p;
    if (m.a16 && epi != EPI_BIAS && epi != EPI_PE) return p;           // only these two read a 16-bit-stored A
    if (m.store16 && epi == EPI_PE) return p;                           // the positional epilogue has no 16-bit-output form
    // latency path: below skinny_rows rows the LDS-tiled kernels cannot fill the chip (measured hand-over,
    // tools/sweep_skinny.py, T=1024, M-A: skinny wins through M = 16384, tiled from 32768).  Exact fp32 with or without the weight
    // copy, fp16x3 with its own copy only; the 16-bit-operand forms are always the LDS-tiled kernels.
    if (m.arith != 1 && M <= skinny_rows && N % 32 == 0 && K % 128 == 0 && (has_wf || m.arith == 0)) {
        p.family = has_wf ? VSK_GEMM_SKINNY2 : VSK_GEMM_SKINNY;
        p.prec = m.arith;
        p.grid_x = (M + 31) / 32;
        p.grid_y = (N + 127) / 128;
        p.lds = has_wf ? vsk_skinny2_lds(K) : 0;
        return p;
    }
    p.family = VSK_GEMM_TILED;
    p.kw = 32;
    if (m.arith == 0) {             // 256x256, 256x128 (N % 256 != 0) or 128x128 tiles
        const bool wide = vsk_use_wide_tiles(M, N);
        p.nwm = wide ? 4 : 2;
        p.nj = wide && N % 256 == 0 ? 4 : 2;
    } else {                        // fp16x3 and every 16-bit form: 256x256 or 128x128 tiles
        const bool big = N % 256 == 0 && M > 128;
        p.nwm = p.nj = big ? 4 : 2;
        p.prec = m.arith == 2 ? 2 : m.f16 ? 3 : 1;
        p.c16 = m.store16;
        p.a16 = m.a16;
        // 64-wide k-tiles from K = 512 up (measured: +6 % on M-B's K = 512 / 2048 products; at K = 256 - four k-tiles per
        // output tile - the 35 registers it spills cost more than the halved barriers give: -4 %), where that instantiation exists
        if (m.arith == 1 && K % 64 == 0 && K >= 512 && vsk_gemm_tuple_legal(epi, p.nwm, p.nj, p.prec, p.c16, 64, p.a16)) p.kw = 64;
    }
    p.ntiles = ((M + 64 * p.nwm - 1) / (64 * p.nwm)) * ((N + 64 * p.nj - 1) / (64 * p.nj));
    p.per_cu = p.nwm == 4 ? 1 : 2;
    return p;
}

// ---- out = LayerNorm(A W^T + bias + res) (+ score head): vsk_linear_res_ln ----
enum VskLnFamily {
    VSK_LN_UNSUPPORTED = 0,
    VSK_LN_SKINNY2,         // skinny2_ln<N / 32, PREC>: latency kernel on the fragment-major weight copy, PREC 0 or 2
    VSK_LN_SKINNY,          // skinny_ln<N / 32>: first generation, exact fp32
    VSK_LN_ROWS,            // gemm_ln_rows<N / 32, PREC, A16>: a lane owns a row, N <= 256, on the row-tile grid
    VSK_LN_RES,             // gemm_res_ln<N / 64, PREC>: the wide kernel, PREC 0 or 2
};

struct VskLnPick {
    VskLnFamily family;
    int width;                      // the kernel's width constant: N / 32 (2, 4, 6, 8), RES: N / 64 (1 .. 8)
    int prec, a16;                  // a16 (PREC 1 only): A is stored as bf16 - here the mode word says so with VSK_STORE16
    int grid, block;                // ROWS: grid 0, the launcher asks vsk_row_tile_grid
    size_t lds;
};

inline VskLnPick vsk_ln_pick(int M, int N, int K, int word, bool has_wf, int skinny_rows) {
    VskLnPick p{};
    const VskLinearMode m = vsk_linear_mode(word);
    if (!m.valid || m.a16 || m.f16) return p;
    const bool narrow = N <= 256 && N % 32 == 0;
    // bf16: the lane-owns-a-row kernels only; fp16x3 has the wide kernel too, from N = 257 up
    if (!narrow && (m.arith == 1 || (m.arith == 2 && N <= 256))) return p;
    p.prec = m.arith;
    p.block = 256;
    if (!narrow) {
        p.width = N / 64;
        if (p.width < 1 || p.width > 8) return p;
        p.family = VSK_LN_RES;
        p.grid = (M + 63) / 64;
        return p;
    }
    p.width = N / 32;
    if (p.width < 2 || p.width % 2) return p;
    if (m.arith != 1 && M <= skinny_rows && K % 128 == 0 && (has_wf || m.arith == 0)) {      // as vsk_gemm_pick
        p.family = has_wf ? VSK_LN_SKINNY2 : VSK_LN_SKINNY;
        p.grid = (M + 31) / 32;
        p.block = 64 * p.width;
        p.lds = has_wf ? vsk_skinny2_lds(K) : 0;
        return p;
    }
    p.family = VSK_LN_ROWS;
    p.a16 = m.store16;
    return p;
}
