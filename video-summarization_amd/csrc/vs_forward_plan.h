// vs_forward_plan.h - which kernels one scoring forward runs: a pure function of the model's shape,
// the call and the switches.  forward_core (vs_scorer.cpp) validates, plans, then only reads the plan.
// Host code, plain C++17, no HIP and no globals: tests/cabi/forward_plan_demo.cpp compiles this header alone.
#pragma once
#include <stddef.h>

#include <cstdio>
#include <string>

#include "vs_scorer.h"      // VS_FLAG_*, VS_ERR_*

// A/B and test switches (DESIGN.md "Environment switches").  Read from the environment ONCE, when the library is
// first used; afterwards only vs_set_option() changes them, so no forward pays a getenv.
struct VskOptions {
    int skinny_rows;      // VS_SKINNY_ROWS   (default 16384)
    int lp_min_rows;      // VS_LP_MIN_ROWS   (default 8192)
    int train_lp_min_rows;// VS_TRAIN_LP_MIN_ROWS (default 1024): frames per batch above which a low-precision TRAINING request is honoured
                          // (profiles/r04_lp_min_rows_sweep.txt: break-even at ~1280 frames, 1.1x at 2560, 1.7x at 8192)
    int lp_min_rows_fused;// VS_LP_MIN_ROWS_FUSED (default 256): the same threshold where the fused bf16 layer kernels apply
    int attn_w64;         // VS_ATTN_W64      (default 1) bf16-stored head-dim-64 attention on the one-wave-per-SIMD kernel (0: the 8-wave kernel, A/B)
    int lp_store32;       // VS_LP_STORE32    bf16 mode keeps q/k/v, the attention output and the MLP hidden tensor fp32 in HBM (A/B)
    int lp_mlp_unfused;   // VS_LP_MLP_UNFUSED bf16 mode runs fc1 and fc2 + LayerNorm as two kernels (A/B)
    int lp_tail_unfused;  // VS_LP_TAIL_UNFUSED bf16 mode runs the out-projection + norm1 as its own kernel in front of the fused MLP (A/B)
    int lp_qkv_unfused;   // VS_LP_QKV_UNFUSED  bf16 mode runs every layer's QKV projection as its own kernel (A/B)
    int lp_tile256;       // VS_LP_TILE256     the fused bf16 layer kernels always use 256-row tiles / 8-wave blocks (A/B)
    int lp_embed_unfused; // VS_LP_EMBED_UNFUSED bf16 mode runs the embedding as the generic GEMM + the first QKV kernel (A/B)
    int exact_unfused;    // VS_EXACT_UNFUSED  exact fp32, d_model 256: out-projection + norm1, fc1, fc2 + norm2 and QKV as four kernels (A/B, bit-identity tests)
    int layer_tail_min_rows; // VS_LAYER_TAIL_MIN_ROWS (default 1024): rows from which the exact fused pair runs as ONE kernel per layer
                          // (vsk_layer_tail; 0 forces it, a value above M keeps the pair; profiles/layer_tail_rows_sweep.txt)
    int mlp_abl;          // VS_MLP_ABL       (diagnostic builds only) timing ablation of the bf16 layer-tail kernel's MLP part (vs_mlp_fused.hip)
    int attn_w64_checked; // VS_ATTN_W64_CHECKED the one-wave-per-SIMD attention skips its optimistic pass (every tile checked; A/B and test pin)
    int attn_w64_abl;     // VS_ATTN_W64_ABL  (diagnostic builds only) timing ablation of the one-wave-per-SIMD attention
};

// kernel mode words (the `mode` / `prec` argument of the launchers in vs_kernels.h): 0 exact, 1 bf16 operands, 2 fp16x3, and on 1
// the bits below; what they mean and which words are valid: vsk_linear_mode (vs_linear_pick.h)
enum { VSK_STORE16 = 16, VSK_A16 = 32, VSK_F16 = 64 };

// kernel-layout weight image families (vsw_ensure, vs_weights_impl.h; the table of DESIGN.md section 42)
enum { VSW_FRAGMENTS = 1, VSW_F16X3 = 2, VSW_BF16 = 4, VSW_ROWS16 = 8,
       // the training backward's: W^T of every matrix row-major (the dgrad GEMMs), the same in fragment-major order (latency
       // kernels), and the bf16 copy of every W2^T (the A-stationary gate GEMM of the bf16 training mode)
       VSW_TRANSPOSED = 16, VSW_TRANSPOSED_FRAGMENTS = 32, VSW_TRANSPOSED_W2_16 = 64,
       VSW_NUM_FAMILIES = 7 };

// ---- which shapes a kernel group takes ----
// the fused bf16 layer kernels of vs_mlp_fused.hip (and their weight images)
inline bool vsk_mlp_bf16_supported(int d) { return d == 256; }
// the bf16-operand GEMM of vs_gemm_ring.hip
inline bool vsk_gemm16_supported(int M, int N, int K) { return M > 0 && N > 0 && N % 32 == 0 && K >= 32 && K % 32 == 0; }
// the exact fused pair layer_outproj_ln_fc1 / layer_fc2_ln_qkv of vs_kernels.hip: throughput batches only
inline bool vsk_layer_fused_supported(int M, int d, int skinny_rows) { return d == 256 && M > skinny_rows && M <= (1 << 20); }
// vsk_attention_packed (vs_attention.hip): the (head dim, waves per block) rows each mode word has a kernel for.  bf16 at head
// dim 128 (both storage forms) has 8-wave blocks only, the exact kernel there 4-wave blocks only; the low-precision
// kernels have no 8-wave form at head dim 32
inline bool vsk_attention_packed_supported(int dh, int nw, int mode) {
    if (nw != 4 && nw != 8) return false;
    if (mode == (1 | VSK_STORE16) || mode == 1) return (dh == 128 && nw == 8) || dh == 64 || (dh == 32 && nw == 4);
    if (mode == 2) return dh == 64 || (dh == 32 && nw == 4);
    if (mode == 0) return (dh == 128 && nw == 4) || dh == 64 || dh == 32;
    return false;
}
// vsk_linear_parts (vs_kernels.hip), latency mode: K in nsplit slices that are multiples of 128, staged in phases of <= 256 k
// (33 KiB of LDS, no opt-in attribute) - a slice above 256 has to be whole phases
inline bool vsk_linear_parts_supported(int N, int K, int nsplit) {
    if (N <= 0 || N % 32 || K <= 0 || nsplit < 1 || K % nsplit) return false;
    const int kslice = K / nsplit;
    return kslice % 128 == 0 && !(kslice > 256 && kslice % 256);
}

// ---- packed ragged batches: the query tile, in waves of 32 rows ----
// r8 / r4: the batch's rows with every video rounded up to 256- / 128-row tiles.  256-row tiles unless the ragged tails
// waste too much; the low-precision attention has no 8-wave form for head dim 32; head dim 128 (round 4): the exact kernel
// has 4-wave blocks, the bf16 one 8-wave blocks only
inline int vs_packed_waves(int dh, int aprec, long long r8, long long r4) {
    if (dh == 128) return aprec == 1 ? 8 : 4;
    return (!(aprec != 0 && dh == 32) && r8 * 100 <= r4 * 105) ? 8 : 4;
}

// ---- the plan ----
enum VsArith { VS_ARITH_EXACT = 0, VS_ARITH_BF16 = 1, VS_ARITH_F16X3 = 2 };      // the values are the kernels' mode words
enum VsEmbedForm {
    VS_EMBED_CLS,        // frames through the embedding GEMM into a free region, then token row + frames -> h0
    VS_EMBED_BF16_QKV,   // vsk_embed_bf16: the bf16 embedding kernel, which also writes the first layer's q/k/v
    VS_EMBED_SPLITK,     // K = in_features split 8 ways, then partials + bias + positional rows -> h0
    VS_EMBED_GEMM,       // vsk_linear
};
enum VsAttentionKernel {
    VS_ATT_PACKED,       // vsk_attention_packed (any precision)
    VS_ATT_DH256,        // head dim 256: the training path's exact forward kernel without dropout
    VS_ATT_SPLITKV,      // latency mode: the keys split over a block's waves
    VS_ATT_LOWPREC,      // vsk_attention_bf16 (bf16 or fp16x3)
    VS_ATT_EXACT,        // vsk_attention
};
enum VsLayerForm {       // everything of a layer behind its attention
    VS_LAYER_RING,       // d_model > 256, bf16: four bf16-operand GEMMs (the QKV included) + two row LayerNorm passes
    VS_LAYER_BF16_TAIL,  // out-projection + norm1 + MLP + norm2 (+ score head) as ONE kernel
    VS_LAYER_BF16_MLP,   // the bf16 out-projection + norm1 kernel (ln1 == VS_LN_FUSED), then the fused MLP kernel
    VS_LAYER_EXACT_PAIR, // exact fp32: out-projection + norm1 + fc1, then fc2 + norm2 (+ the next layer's QKV)
    VS_LAYER_STAGES,     // out-projection + norm1 as `ln1`, fc1, fc2 + norm2 as `ln2`
};
enum VsLnForm {          // a Linear + residual + LayerNorm that is a stage of its own
    VS_LN_NONE,          // (part of a larger kernel in this layer form)
    VS_LN_SPLITK_ROWS,   // split-K partial products, then the row pass that sums them
    VS_LN_GEMM_ROWS,     // plain GEMM, then the row pass
    VS_LN_FUSED,         // vsk_linear_res_ln
};

struct VsForwardIn {
    int d_model, num_heads, num_layers, in_features, max_len;      // vs_model_desc
    int norm_width;             // LayerNorm width; != d_model: a narrower model embedded in this shape
    bool has_pe, has_b_embed;   // a positional table; the bf16 embedding kernel's weight image exists
    int B, T;                   // T: frames per video (a packed batch: B = 1, T = all frames)
    unsigned flags;             // VS_FLAG_*
    bool cls, packed;           // class token prepended; vs_scorer_forward_packed
};

struct VsForwardPlan {
    int T, M;                   // positions per video the encoder sees (frames + class token), rows = B * T
    VsArith linear, attention_arith;
    unsigned families;          // VSW_*: the weight images this forward reads
    VsEmbedForm embed;
    VsAttentionKernel attention;
    VsLayerForm layer;
    VsLnForm ln1, ln2;
    // bf16 mode: the tensors that are only ever read as bf16 matrix operands are WRITTEN as bf16 by their producers
    // (q * scale * log2 e, k, v and the attention output: qkv16; the MLP hidden tensor: ffn16) - same bits, half the HBM bytes
    bool qkv16, ffn16;
    bool next_qkv;              // the bf16 layer kernels also project their output rows to the NEXT layer's q/k/v
    size_t kv_stride;           // floats between the q, k and v planes: M * d, or half of it where they are bf16 planes
    int mode_linear;            // mode word of the embedding, the plain and the split-K GEMMs
    int mode_qkv;               // ... of vsk_qkv and of the out-projection + norm1 (whose A is the attention output)
    int mode_ffn;               // ... of fc1 and fc2 + norm2 (the MLP hidden tensor between them)
    int mode_attention;         // ... of the packed and the low-precision attention

    // q/k/v of layer l > 0 were written by the closing kernel of layer l - 1 (layer 0: embed == VS_EMBED_BF16_QKV)
    bool tail_writes_qkv() const { return next_qkv || layer == VS_LAYER_EXACT_PAIR; }
};

inline int vs_attention_prec(unsigned flags) { return (flags & VS_FLAG_F16X3_ATTENTION) ? 2 : (flags & VS_FLAG_BF16_ATTENTION) ? 1 : 0; }

// VS_OK and *plan, or the error code and its text in *err (plan untouched)
inline int vs_forward_plan(const VsForwardIn &in, const VskOptions &opt, VsForwardPlan *plan, std::string *err) {
    char msg[192];
    auto fail = [&](int code) { *err = msg; return code; };
    const int d = in.d_model, H = in.num_heads, dh = d / H;
    const unsigned flags = in.flags;
    if (!in.packed && in.has_pe && in.T > in.max_len) {
        snprintf(msg, sizeof msg, "T=%d exceeds the positional table (max_len=%d)", in.T, in.max_len);
        return fail(VS_ERR_INVALID);
    }
    if (in.cls && in.packed) { snprintf(msg, sizeof msg, "packed batches have no class-token form"); return fail(VS_ERR_INVALID); }
    const int T = in.T + (in.cls ? 1 : 0);      // sequence length the encoder sees
    if ((long long)in.B * T > (1ll << 30)) { snprintf(msg, sizeof msg, "B*T too large"); return fail(VS_ERR_INVALID); }
    if ((flags & VS_FLAG_BF16_LINEAR) && (flags & VS_FLAG_F16X3_LINEAR)) {
        snprintf(msg, sizeof msg, "VS_FLAG_BF16_LINEAR and VS_FLAG_F16X3_LINEAR are exclusive");
        return fail(VS_ERR_INVALID);
    }
    if ((flags & (VS_FLAG_BF16_ATTENTION | VS_FLAG_F16X3_ATTENTION)) && dh != 32 && dh != 64 && !((flags & VS_FLAG_BF16_ATTENTION) && dh == 128)) {
        snprintf(msg, sizeof msg, "VS_FLAG_BF16_ATTENTION needs head_dim 32, 64 or 128, VS_FLAG_F16X3_ATTENTION 32 or 64 (got %d)", dh);
        return fail(VS_ERR_INVALID);
    }
    if ((flags & VS_FLAG_BF16_ATTENTION) && (flags & VS_FLAG_F16X3_ATTENTION)) {
        snprintf(msg, sizeof msg, "VS_FLAG_BF16_ATTENTION and VS_FLAG_F16X3_ATTENTION are exclusive");
        return fail(VS_ERR_INVALID);
    }

    VsForwardPlan p{};
    p.T = T;
    p.M = in.B * T;
    const int M = p.M;
    const bool embedded = in.norm_width != d;      // (an embedded model's LayerNorm width is not d: only the row pass knows it)
    const int aprec = vs_attention_prec(flags);
    p.attention_arith = (VsArith)aprec;
    // bf16 Linear kernels exist as LDS-tiled throughput kernels only: up to 8192 rows (measured crossover) the exact
    // fp32 latency kernels are faster and are used whatever that flag says.  fp16x3 has its own latency kernels
    // (same product order as its tiled kernels: a video's scores do not depend on the batch it is scored in).
    // (measured crossover, T=1024: 8192 rows for the stand-alone bf16 GEMMs; where the fused layer kernels of
    // vs_mlp_fused.hip apply - d_model 256 with bf16 attention - they win from a single T=320 video on (128-row tiles on
    // 4-wave blocks below half a chip of 256-row tiles: 0.36 ms at 320 rows, 0.43 ms from 1k to 8k rows): 256 rows)
    const bool fused_ok = !embedded && vsk_mlp_bf16_supported(d) && aprec == 1 && !opt.lp_store32 && !opt.lp_mlp_unfused;
    const int lp_min_rows = fused_ok && opt.lp_min_rows_fused < opt.lp_min_rows ? opt.lp_min_rows_fused
                                                                               : opt.lp_min_rows;    // tests / tools pin the bf16 tiled kernels with 0
    p.linear = (flags & VS_FLAG_F16X3_LINEAR) ? VS_ARITH_F16X3 : ((flags & VS_FLAG_BF16_LINEAR) && M > lp_min_rows) ? VS_ARITH_BF16 : VS_ARITH_EXACT;
    const bool bf16 = p.linear == VS_ARITH_BF16;
    // latency mode (VS_FLAG_SPLITK): exact or fp16x3 kernels, latency-sized inputs, plain padded batches only
    // (d_model 128 .. 512 - M-A and the reference's argparse default M-B: K slices that are multiples of 128, partials in the free regions;
    // the slices of fc2, K = 4 d in four, and from d_model 256 on of the out-projection, K = d in two, are ones vsk_linear_parts takes)
    const bool splitk = (flags & VS_FLAG_SPLITK) && !bf16 && !in.packed && !in.cls && M <= opt.skinny_rows && (d == 128 || d == 256 || d == 512) &&
                        vsk_linear_parts_supported(d, 4 * d, 4) && (d < 256 || vsk_linear_parts_supported(d, d, 2));
    // weight images: bf16 mode reads the LDS images (d_model > 256: the bf16-operand GEMM's row-major copies too); the other
    // modes read the fragment-major copies wherever a GEMM of this forward is small enough for the latency kernels
    const int rows_min = in.cls ? in.B * in.T : M;
    p.families = 0;
    if (bf16) p.families = VSW_BF16;
    else if (rows_min <= opt.skinny_rows) p.families = p.linear == VS_ARITH_F16X3 ? VSW_F16X3 : VSW_FRAGMENTS;
    if (bf16 && d > 256) p.families |= VSW_ROWS16;
    // (d_model > 256 - M-B and wider - has no bf16-storage consumers: its LayerNorm GEMMs are the plain bf16 GEMM + the
    // row pass, which read fp32, and the head-dim-128 attention reads fp32 q / k / v: fp32 storage there)
    p.ffn16 = bf16 && d <= 256 && !embedded && !opt.lp_store32;
    p.qkv16 = p.ffn16 && aprec == 1;
    const bool mlp16 = bf16 && !embedded && vsk_mlp_bf16_supported(d) && !opt.lp_mlp_unfused && !opt.lp_store32;
    // d_model > 256 in bf16 mode with a bf16 attention: the bf16-OPERAND GEMM (vs_gemm_ring.hip).  Every Linear after the
    // embedding reads bf16 from HBM: q/k/v, the attention output and the MLP hidden tensor are written as bf16 by their
    // producers, and the two LayerNorm passes write a bf16 copy of their rows beside the fp32 residual stream.
    const bool ring = bf16 && aprec == 1 && !in.packed && d > 256 && !opt.lp_store32 && vsk_gemm16_supported(M, d, d);
    p.kv_stride = (p.qkv16 || ring) ? (size_t)M * d / 2 : (size_t)M * d;
    // bf16 mode with bf16 q/k/v: every layer's tail kernel also projects its output rows to the NEXT layer's q/k/v, and
    // the embedding kernel to the first layer's
    p.next_qkv = mlp16 && p.qkv16 && !opt.lp_qkv_unfused;
    // exact fp32, d_model 256, throughput batches: out-projection + norm1 carries fc1, and fc2 + norm2 the NEXT layer's QKV, each
    // fed from the registers that hold the rows it has just normalised (vs_kernels.hip: LnTail) - bit-identical to the four
    // stand-alone kernels, which VS_EXACT_UNFUSED=1 brings back.  The first layer's QKV stays vsk_qkv.
    const bool exact_fused = p.linear == VS_ARITH_EXACT && aprec == 0 && !embedded && !splitk && !opt.exact_unfused &&
                             vsk_layer_fused_supported(M, d, opt.skinny_rows) && d % H == 0 && dh % 32 == 0;

    p.embed = in.cls ? VS_EMBED_CLS
            : bf16 && in.has_b_embed && p.next_qkv && in.num_layers > 0 && !opt.lp_embed_unfused ? VS_EMBED_BF16_QKV
            : splitk && vsk_linear_parts_supported(d, in.in_features, 8) ? VS_EMBED_SPLITK     // (in_features 3072, 5120: the default kernels)
            : VS_EMBED_GEMM;
    p.attention = in.packed ? VS_ATT_PACKED
                : dh == 256 ? VS_ATT_DH256       // (round 4, correctness first)
                : splitk && aprec != 1 && (dh == 32 || dh == 64 || dh == 128) ? VS_ATT_SPLITKV
                : aprec ? VS_ATT_LOWPREC
                : VS_ATT_EXACT;
    // d_model > 256 or an embedded model: plain GEMM + the row LayerNorm pass (faster than the fused wide kernel at every M);
    // latency mode: K = d in two slices from d_model 256 on, K = 4 d in four at every width
    const VsLnForm ln = (d > 256 || embedded) ? VS_LN_GEMM_ROWS : VS_LN_FUSED;
    p.ln1 = p.ln2 = VS_LN_NONE;
    if (ring) p.layer = VS_LAYER_RING;
    else if (mlp16 && p.qkv16 && !opt.lp_tail_unfused) p.layer = VS_LAYER_BF16_TAIL;
    else if (exact_fused) p.layer = VS_LAYER_EXACT_PAIR;
    else {
        p.layer = mlp16 ? VS_LAYER_BF16_MLP : VS_LAYER_STAGES;
        p.ln1 = splitk && d >= 256 ? VS_LN_SPLITK_ROWS : ln;
        if (!mlp16) p.ln2 = splitk ? VS_LN_SPLITK_ROWS : ln;
    }
    p.mode_linear = p.linear;
    p.mode_qkv = p.qkv16 ? (1 | VSK_STORE16) : p.linear;
    p.mode_ffn = p.ffn16 ? (1 | VSK_STORE16) : p.linear;
    p.mode_attention = (p.qkv16 || ring) ? (1 | VSK_STORE16) : aprec;
    // the plan names only kernels that exist: a packed batch's tiling is a fact of its lengths (vs_packed_waves), so both
    // tilings this head dim and arithmetic can get must have a kernel in this mode
    if (in.packed)
        for (long long r8 = 1; r8 <= 2; ++r8)
            if (!vsk_attention_packed_supported(dh, vs_packed_waves(dh, aprec, r8, 1), p.mode_attention)) {
                if (dh != 32 && dh != 64 && dh != 128) snprintf(msg, sizeof msg, "packed batches need head_dim 32, 64 or 128 (got %d)", dh);
                else snprintf(msg, sizeof msg, "packed batches: no attention kernel for head_dim %d in mode %d", dh, p.mode_attention);
                return fail(VS_ERR_INVALID);
            }
    *plan = p;
    return VS_OK;
}
