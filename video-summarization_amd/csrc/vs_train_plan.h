// vs_train_plan.h - the form of one training call's activation record and the mode word of every launch that reads or writes
// it: a pure function of the model's shape, the call, the dropout config and the switches.
// forward_impl / backward_impl (vs_train.cpp) check their pointers, plan, then only read the plan.
// Host code, plain C++17, no HIP and no globals: tests/cabi/train_plan_demo.cpp compiles this header alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstdio>
#include <string>

#include "vs_forward_plan.h"      // VskOptions, VSK_* mode bits, VSW_* image families
#include "vs_train.h"             // VS_TRAIN_FLAG_*

// vst_wgrad prec = 1 | flag: dY / X is stored as a 16-bit tensor
enum { VST_WGRAD_Y16 = 2, VST_WGRAD_X16 = 4 };

// ---- which shapes a kernel group takes ----
// the attention on the bf16 / fp16 matrix pipe (vs_train_attention_bf16.hip), padded and packed
inline bool vst_attention_bf16_supported(int dh) { return dh == 32 || dh == 64 || dh == 128; }
// the A-stationary bf16 GEMM (vs_train_gemm_rows.hip).  By itself from 3/4 of a 256-row block per CU up (the grid is M / 256
// blocks: at 16 384 rows it would fill a quarter of the chip and measured 7 % slower per step than the tiled kernels' 256
// tiles); MI355X: 256 CUs.  any_rows: the kernel itself handles every M - tests pin it on small batches
inline bool vst_gemm_rows16_supported(int M, int N, int K, bool any_rows = false) {
    return (K == 256 || K == 512) && N % 8 == 0 && N >= 64 && N <= 4096 && M > 0 && (any_rows || M >= 192 * 256);
}

// ---- the FORM of an activation record: which tensors of it are 16-bit planes / which arithmetic wrote it ----
// The forward derives it from the request (vs_dropout_cfg.flags), the batch size and the switches; the backward must read the
// record in the form it was WRITTEN in.  The forward therefore publishes the form (vs_train_last_format(), per calling thread)
// and the backward takes it back through vs_dropout_cfg.reserved - a switch flipped between the two calls (another model, a
// retained graph, a test) cannot make the backward read bf16 planes as fp32.  reserved == 0: derived again (older callers).
struct VsTrainForm {
    bool lp, lpa;         // Linear / dgrad / wgrad GEMMs, the attention products: on the 16-bit matrix pipe
    bool qkv16, h16;      // q / k / v (and dO, dq | dk | dv), the MLP hidden tensor (and its gradient): stored as 16-bit planes
    bool rows16;          // fc1, the gated fc2 input gradient (and, with qkv16, the QKV projection) on the A-stationary kernel
    bool f16;             // the 16-bit type of everything above is IEEE f16 (VS_TRAIN_FLAG_FP16), not bf16
};
inline bool operator==(const VsTrainForm &a, const VsTrainForm &b) {
    return a.lp == b.lp && a.lpa == b.lpa && a.qkv16 == b.qkv16 && a.h16 == b.h16 && a.rows16 == b.rows16 && a.f16 == b.f16;
}
// the published word (ABI: Python and the tests read bits 0, 1, 4 and 5) and its inverse; bit 31 says "a form, not 0"
enum : uint32_t { VST_FORM_VALID = 0x80000000u, VST_FORM_BITS = 0x3fu };
inline uint32_t vs_train_form_bits(const VsTrainForm &f) {
    return VST_FORM_VALID | (f.lp ? 1u : 0u) | (f.lpa ? 2u : 0u) | (f.qkv16 ? 4u : 0u) | (f.h16 ? 8u : 0u) | (f.rows16 ? 16u : 0u) | (f.f16 ? 32u : 0u);
}
inline VsTrainForm vs_train_form_parse(uint32_t bits) {
    return VsTrainForm{(bits & 1u) != 0, (bits & 2u) != 0, (bits & 4u) != 0, (bits & 8u) != 0, (bits & 16u) != 0, (bits & 32u) != 0};
}

// ---- the plan ----
enum VsTrainAttention {
    VST_ATT_PACKED16,     // vst_attention_fwd / bwd_bf16_packed: fp32-stored planes, 16-bit products
    VST_ATT_PACKED_EXACT, // vst_attention_fwd / bwd_packed
    VST_ATT_PADDED16,     // vst_attention_fwd / bwd_bf16 (planes stored as fp32, or as 16-bit with qkv16)
    VST_ATT_PADDED_EXACT, // vst_attention_fwd / bwd
};

struct VsTrainIn {
    int d_model, num_heads, max_len;      // vs_model_desc
    bool has_pe;                          // a positional table
    int B, T;                             // a packed batch: B = 1, T = all frames
    bool packed;
    unsigned flags; float p, p_embed; unsigned reserved;      // vs_dropout_cfg (all 0 when the call has none)
    bool backward;
};

struct VsTrainPlan {
    VsTrainForm form;
    uint32_t format;            // vs_train_form_bits(form): what vs_train_last_format() publishes
    VsTrainAttention attention;
    size_t kv_stride;           // floats between the q, k and v planes: M * d, or half of it where they are 16-bit planes
    bool qkv_rows16;            // the QKV projection runs on the A-stationary kernel
    unsigned families;          // forward: the VSW_* weight images to ensure
    bool transposed_fragments;  // backward: the fragment-major copies of W^T too (latency kernels)
    bool t16;                   // backward: the bf16 copy of every W2^T (the A-stationary gate GEMM's weight operand)
    // One mode word per launch site, named after the tensor it describes.  0 exact; 1 16-bit operands (| VSK_F16: f16);
    // VSK_STORE16 / VSK_A16 / VST_WGRAD_*16: that tensor lives in HBM as a 16-bit plane.
    int mode_linear;            // embedding, out-projection, their wgrads and dgrads: every operand fp32-stored
    int mode_qkv;               // vsk_qkv writes q / k / v
    int mode_fc1, mode_fc2;     // fc1 writes the MLP hidden tensor, fc2 reads it
    int mode_attention;         // in16 of the padded 16-bit attention, forward AND backward: q / k / v stored as 16-bit
    bool attention_out16;       // ... and its backward writes dq | dk | dv as 16-bit
    int mode_rowdot;            // vst_head_rowdot: 1 dO stored as 16-bit, 2 fp32 dO rounded in the dot, 0 exact
    int mode_wgrad_w2;          // X = the MLP hidden tensor
    int mode_gate;              // vsk_linear_gate writes the hidden tensor's gradient
    int mode_wgrad_w1;          // dY = that gradient
    int mode_dgrad_fc1;         // A = that gradient
    int mode_datt;              // the out-projection's dgrad writes dO
    int mode_wgrad_qkv;         // dY = dq | dk | dv
    int mode_dgrad_qkv;         // A = dq | dk | dv
};

// the form a forward writes
inline VsTrainForm vs_train_derive_form(const VsTrainIn &in, const VskOptions &opt) {
    VsTrainForm f{};
    const long long rows = (long long)in.B * in.T;
    // low-precision training (VS_TRAIN_FLAG_BF16_LINEAR): every Linear / dgrad / wgrad GEMM on the bf16 matrix pipe, from the
    // batch size up where that pays (VS_TRAIN_LP_MIN_ROWS, default 1024 frames: tools/sweep_lp_min_rows.py,
    // profiles/r04_lp_min_rows_sweep.txt - break-even at ~1280 frames, never slower; rounds 2-3 used the scoring path's 8192)
    f.lp = (in.flags & VS_TRAIN_FLAG_BF16_LINEAR) && rows > opt.train_lp_min_rows;
    // ... and (VS_TRAIN_FLAG_BF16_ATTENTION) the attention products of the forward and the backward (head dim 32 / 64 / 128)
    // (packed ragged batches: the attention stays exact fp32 unless VS_TRAIN_FLAG_PACKED_LP_ATTENTION opts in as well - the
    // padded rule counted on the packed rows, B * T = Mtot here; padded calls do not read that bit)
    f.lpa = (in.flags & VS_TRAIN_FLAG_BF16_ATTENTION) && (!in.packed || (in.flags & VS_TRAIN_FLAG_PACKED_LP_ATTENTION)) &&
            rows > opt.train_lp_min_rows && vst_attention_bf16_supported(in.d_model / in.num_heads);
    // 16-bit STORAGE of the tensors that are only ever 16-bit matrix operands (VS_LP_STORE32 = 1 keeps them fp32: an A/B switch -
    // the kernels round the fp32-stored values to the same 16 bits, so every result is bit-identical either way)
    // (packed: the packed 16-bit attention kernels read fp32-stored planes and an fp32 dO only)
    f.qkv16 = !in.packed && f.lp && f.lpa && !opt.lp_store32;
    f.h16 = f.lp && !opt.lp_store32;
    f.f16 = (f.lp || f.lpa) && (in.flags & VS_TRAIN_FLAG_FP16) != 0;
    // the A-stationary GEMM writes the hidden tensor where it applies (K = d_model = 256 / 512, batches that fill the chip;
    // VS_LP_MLP_UNFUSED = 1: the tiled kernels, 2: the A-stationary kernel at every batch size - A/B and test switches).  It
    // and its pre-rounded weight copies exist in bf16 only: the fp16 mode runs the tiled GEMMs
    f.rows16 = f.h16 && !f.f16 && opt.lp_mlp_unfused != 1 &&
               vst_gemm_rows16_supported(in.B * in.T, 4 * in.d_model, in.d_model, opt.lp_mlp_unfused == 2);
    return f;
}

// can a record of this model / batch have the form that `bits` (a caller's vs_dropout_cfg.reserved) spells?
inline bool vs_train_form_possible(uint32_t bits, const VsTrainIn &in) {
    const VsTrainForm f = vs_train_form_parse(bits);
    return !((f.qkv16 && !(f.lp && f.lpa)) || (f.h16 && !f.lp) || (f.rows16 && !f.h16) || (f.f16 && (f.rows16 || !(f.lp || f.lpa))) ||
             (bits & ~(VST_FORM_VALID | VST_FORM_BITS)) || (in.packed && f.qkv16) ||
             (f.lpa && !vst_attention_bf16_supported(in.d_model / in.num_heads)) ||
             (f.rows16 && !vst_gemm_rows16_supported(in.B * in.T, 4 * in.d_model, in.d_model, true)));
}

// VS_OK and *plan, or the error code and its text in *err (plan untouched)
inline int vs_train_plan(const VsTrainIn &in, const VskOptions &opt, VsTrainPlan *plan, std::string *err) {
    char msg[192];
    auto fail = [&](int code) { *err = msg; return code; };
    if (in.B <= 0 || in.T <= 0) { snprintf(msg, sizeof msg, "B=%d T=%d", in.B, in.T); return fail(VS_ERR_INVALID); }
    if ((long long)in.B * in.T > (1ll << 28)) { snprintf(msg, sizeof msg, "B*T too large"); return fail(VS_ERR_INVALID); }
    if (!in.packed && in.has_pe && in.T > in.max_len) {
        snprintf(msg, sizeof msg, "T=%d exceeds the positional table (max_len=%d)", in.T, in.max_len);
        return fail(VS_ERR_INVALID);
    }
    if (in.p < 0.f || in.p >= 1.f || in.p_embed < 0.f || in.p_embed >= 1.f) {
        snprintf(msg, sizeof msg, "dropout probabilities must be in [0, 1): p=%g p_embed=%g", in.p, in.p_embed);
        return fail(VS_ERR_INVALID);
    }

    VsTrainPlan p{};
    // the form the record was written in: handed back by the caller (vs_dropout_cfg.reserved = vs_train_last_format() of the
    // forward), else derived from the same inputs the forward had.  The forward does not read `reserved`.
    if (in.backward && (in.reserved & VST_FORM_VALID)) {
        if (!vs_train_form_possible(in.reserved, in)) {
            snprintf(msg, sizeof msg, "vs_dropout_cfg.reserved = 0x%08x is not a record form this model / batch can have", in.reserved);
            return fail(VS_ERR_INVALID);
        }
        p.form = vs_train_form_parse(in.reserved);
    } else {
        p.form = vs_train_derive_form(in, opt);
    }
    const VsTrainForm &f = p.form;
    p.format = vs_train_form_bits(f);
    p.attention = in.packed ? (f.lpa ? VST_ATT_PACKED16 : VST_ATT_PACKED_EXACT) : (f.lpa ? VST_ATT_PADDED16 : VST_ATT_PADDED_EXACT);
    const size_t plane = (size_t)in.B * in.T * in.d_model;
    p.kv_stride = f.qkv16 ? plane / 2 : plane;
    p.qkv_rows16 = f.rows16 && f.qkv16;
    // weight images: the fragment-major copies (of W, and in the backward of W^T) wherever the batch is small enough for the
    // latency kernels; the bf16 row-major copies (of W1 / Wqkv, and in the backward of W2^T) for the A-stationary kernel
    const bool skinny = in.B * in.T <= opt.skinny_rows;
    if (in.backward) { p.transposed_fragments = skinny; p.t16 = f.rows16; }
    else p.families = (skinny ? (unsigned)VSW_FRAGMENTS : 0u) | (f.rows16 ? (unsigned)VSW_ROWS16 : 0u);

    const int F = f.f16 ? VSK_F16 : 0;      // fp16 mode: rides on every 16-bit mode word
    const int lp = f.lp ? (1 | F) : 0;
    p.mode_linear = lp;
    // q (times scale * log2 e), k, v are WRITTEN as 16-bit by the QKV GEMM's epilogue - the attention kernels' only readers round
    // them anyway: same bits, half the saved bytes.  dO and dq | dk | dv likewise: only ever operands of 16-bit products
    p.mode_qkv = f.qkv16 ? (1 | VSK_STORE16 | F) : lp;
    p.mode_attention = (f.qkv16 ? 1 : 0) | F;
    p.attention_out16 = f.qkv16;
    p.mode_datt = f.qkv16 ? (1 | VSK_STORE16 | F) : lp;
    // (delta is the row dot of the SAME rounded dO the attention backward multiplies with the saved fp32 output)
    p.mode_rowdot = f.qkv16 ? (1 | F) : f.lpa ? (2 | F) : 0;
    p.mode_wgrad_qkv = f.qkv16 ? (1 | VST_WGRAD_Y16 | F) : lp;
    p.mode_dgrad_qkv = f.qkv16 ? (1 | VSK_A16 | F) : lp;
    // the MLP hidden tensor (post ReLU, post dropout) is only ever a matrix operand or a sign, its gradient only an operand
    p.mode_fc1 = f.h16 ? (1 | VSK_STORE16 | F) : lp;
    p.mode_fc2 = f.h16 ? (1 | VSK_A16 | F) : lp;
    p.mode_wgrad_w2 = f.h16 ? (1 | VST_WGRAD_X16 | F) : lp;
    p.mode_gate = f.h16 ? (1 | VSK_STORE16 | F) : lp;
    p.mode_wgrad_w1 = f.h16 ? (1 | VST_WGRAD_Y16 | F) : lp;
    p.mode_dgrad_fc1 = f.h16 ? (1 | VSK_A16 | F) : lp;
    *plan = p;
    return VS_OK;
}
