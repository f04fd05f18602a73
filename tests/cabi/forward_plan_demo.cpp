// csrc/vs_forward_plan.h alone, as plain C++17 (no HIP): tests/test_forward_plan_host.py builds this with the host compiler and
// -fsanitize=address,undefined.  Part 1: named cases -> the expected plan (every enumerator of every plan enum is reached);
// part 2: what each A/B switch flips; part 3: invariants and the refusals over a grid, and for every accepted
// plan the support predicate of each kernel it names (kernels_exist).
// Prints "OK" or the first failed check.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <utility>

#include "vs_forward_plan.h"

#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAILED line %d: %s\n", __LINE__, #__VA_ARGS__); return 1; } } while (0)

namespace {

const int S16 = 1 | VSK_STORE16;
const unsigned BF16 = VS_FLAG_BF16, BF16_LIN = VS_FLAG_BF16_LINEAR, BF16_ATT = VS_FLAG_BF16_ATTENTION, F16X3 = VS_FLAG_F16X3, SPLITK = VS_FLAG_SPLITK;

VskOptions defaults() {
    VskOptions o{};
    o.skinny_rows = 16384; o.lp_min_rows = 8192; o.lp_min_rows_fused = 256; o.train_lp_min_rows = 1024; o.attn_w64 = 1;
    return o;
}

// d_model, heads, 4 layers, in_features 1024, a positional table of 20000 rows; the bf16 embedding image exists for d_model 256
VsForwardIn model(int d, int heads, int in_features = 1024) {
    return VsForwardIn{d, heads, 4, in_features, 20000, d, true, d == 256 && in_features % 64 == 0, 1, 1, 0u, false, false};
}
VsForwardIn call(VsForwardIn m, int B, int T, unsigned flags) { m.B = B; m.T = T; m.flags = flags; return m; }
VsForwardIn rows(VsForwardIn m, int n, unsigned flags) { return call(m, 1, n, flags); }
VsForwardIn with_cls(VsForwardIn m) { m.cls = true; return m; }
VsForwardIn packed(VsForwardIn m) { m.packed = true; return m; }
VsForwardIn embedded(VsForwardIn m) { m.norm_width = m.d_model - 4; return m; }
const VsForwardIn MA = model(256, 4);       // M-A: d_model 256, 4 heads (head dim 64), 4 layers

enum Field { F_T, F_M, F_LINEAR, F_ATT_ARITH, F_FAMILIES, F_EMBED, F_ATTENTION, F_LAYER, F_LN1, F_LN2, F_QKV16, F_FFN16, F_NEXT_QKV, F_KV_STRIDE,
             F_MODE_LINEAR, F_MODE_QKV, F_MODE_FFN, F_MODE_ATT, F_COUNT };
unsigned bit(Field f) { return 1u << f; }
// the fields in which two plans differ
unsigned differing(const VsForwardPlan &a, const VsForwardPlan &b) {
    unsigned m = 0;
    if (a.T != b.T) m |= bit(F_T);
    if (a.M != b.M) m |= bit(F_M);
    if (a.linear != b.linear) m |= bit(F_LINEAR);
    if (a.attention_arith != b.attention_arith) m |= bit(F_ATT_ARITH);
    if (a.families != b.families) m |= bit(F_FAMILIES);
    if (a.embed != b.embed) m |= bit(F_EMBED);
    if (a.attention != b.attention) m |= bit(F_ATTENTION);
    if (a.layer != b.layer) m |= bit(F_LAYER);
    if (a.ln1 != b.ln1) m |= bit(F_LN1);
    if (a.ln2 != b.ln2) m |= bit(F_LN2);
    if (a.qkv16 != b.qkv16) m |= bit(F_QKV16);
    if (a.ffn16 != b.ffn16) m |= bit(F_FFN16);
    if (a.next_qkv != b.next_qkv) m |= bit(F_NEXT_QKV);
    if (a.kv_stride != b.kv_stride) m |= bit(F_KV_STRIDE);
    if (a.mode_linear != b.mode_linear) m |= bit(F_MODE_LINEAR);
    if (a.mode_qkv != b.mode_qkv) m |= bit(F_MODE_QKV);
    if (a.mode_ffn != b.mode_ffn) m |= bit(F_MODE_FFN);
    if (a.mode_attention != b.mode_attention) m |= bit(F_MODE_ATT);
    return m;
}

// one row of the table: what the plan must say (T, M and kv_stride follow from the call: `kv_half`)
struct Want {
    VsArith linear, attention_arith;
    unsigned families;
    VsEmbedForm embed;
    VsAttentionKernel attention;
    VsLayerForm layer;
    VsLnForm ln1, ln2;
    bool qkv16, ffn16, next_qkv, kv_half;
    int mode_linear, mode_qkv, mode_ffn, mode_attention;
};
struct Case { const char *name; VsForwardIn in; VskOptions opt; Want want; };

std::set<std::pair<int, int>> g_seen;       // (enum, enumerator) reached by a named case

bool plan_is(const Case &c) {
    VsForwardPlan p;
    std::string err;
    if (vs_forward_plan(c.in, c.opt, &p, &err) != VS_OK) { std::printf("%s: refused: %s\n", c.name, err.c_str()); return false; }
    const Want &w = c.want;
    const int T = c.in.T + (c.in.cls ? 1 : 0);
    const size_t plane = (size_t)c.in.B * T * c.in.d_model;
    const VsForwardPlan e{T, c.in.B * T, w.linear, w.attention_arith, w.families, w.embed, w.attention, w.layer, w.ln1, w.ln2, w.qkv16, w.ffn16,
                          w.next_qkv, w.kv_half ? plane / 2 : plane, w.mode_linear, w.mode_qkv, w.mode_ffn, w.mode_attention};
    if (const unsigned m = differing(p, e)) { std::printf("%s: plan differs from the table in fields 0x%x\n", c.name, m); return false; }
    g_seen.insert({0, p.linear}); g_seen.insert({1, p.attention_arith}); g_seen.insert({2, p.embed}); g_seen.insert({3, p.attention});
    g_seen.insert({4, p.layer}); g_seen.insert({5, p.ln1}); g_seen.insert({5, p.ln2});
    return true;
}

VskOptions with(int VskOptions::*field, int value) { VskOptions o = defaults(); o.*field = value; return o; }

// ---- part 1: the table ----
const Want EXACT_STAGES{VS_ARITH_EXACT, VS_ARITH_EXACT, VSW_FRAGMENTS, VS_EMBED_GEMM, VS_ATT_EXACT, VS_LAYER_STAGES, VS_LN_FUSED, VS_LN_FUSED,
                        false, false, false, false, 0, 0, 0, 0};
// bf16 Linear + bf16 attention on M-A: the fused layer kernels, everything operand-only stored as bf16
const Want BF16_FUSED{VS_ARITH_BF16, VS_ARITH_BF16, VSW_BF16, VS_EMBED_BF16_QKV, VS_ATT_LOWPREC, VS_LAYER_BF16_TAIL, VS_LN_NONE, VS_LN_NONE,
                      true, true, true, true, 1, S16, S16, S16};
// bf16 Linear with the exact attention on M-A: fp32 q/k/v, so the out-projection is its own kernel in front of the fused MLP
const Want BF16_LIN_MA{VS_ARITH_BF16, VS_ARITH_EXACT, VSW_BF16, VS_EMBED_GEMM, VS_ATT_EXACT, VS_LAYER_BF16_MLP, VS_LN_FUSED, VS_LN_NONE,
                       false, true, false, false, 1, 1, S16, 0};
const Want RING{VS_ARITH_BF16, VS_ARITH_BF16, VSW_BF16 | VSW_ROWS16, VS_EMBED_GEMM, VS_ATT_LOWPREC, VS_LAYER_RING, VS_LN_NONE, VS_LN_NONE,
                false, false, false, true, 1, 1, 1, S16};
const Want WIDE_BF16_LIN{VS_ARITH_BF16, VS_ARITH_EXACT, VSW_BF16 | VSW_ROWS16, VS_EMBED_GEMM, VS_ATT_EXACT, VS_LAYER_STAGES, VS_LN_GEMM_ROWS,
                         VS_LN_GEMM_ROWS, false, false, false, false, 1, 1, 1, 0};

Want but(Want w, void (*change)(Want &)) { change(w); return w; }

const Case kCases[] = {
    {"M-A, one T=320 video, exact", rows(MA, 320, 0), defaults(), EXACT_STAGES},
    // bf16 Linear flag alone (exact attention): the stand-alone bf16 GEMMs' threshold, VS_LP_MIN_ROWS
    {"M-A, bf16 Linear at lp_min_rows: exact kernels", rows(MA, 8192, BF16_LIN), defaults(), EXACT_STAGES},
    {"M-A, bf16 Linear at lp_min_rows + 1", rows(MA, 8193, BF16_LIN), defaults(), BF16_LIN_MA},
    // with the bf16 attention the fused layer kernels apply: VS_LP_MIN_ROWS_FUSED
    {"M-A, bf16 at lp_min_rows_fused: exact Linear kernels, bf16 attention", rows(MA, 256, BF16), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.attention_arith = VS_ARITH_BF16; w.attention = VS_ATT_LOWPREC; w.mode_attention = 1; })},
    {"M-A, bf16 at lp_min_rows_fused + 1", rows(MA, 257, BF16), defaults(), BF16_FUSED},
    {"M-A, bf16, B=8 x T=1024", call(MA, 8, 1024, BF16), defaults(), BF16_FUSED},
    // the latency kernels and their fragment-major weights end at VS_SKINNY_ROWS; the exact fused pair begins above it
    {"M-A, exact at skinny_rows", rows(MA, 16384, 0), defaults(), EXACT_STAGES},
    {"M-A, exact at skinny_rows + 1", rows(MA, 16385, 0), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.families = 0; w.layer = VS_LAYER_EXACT_PAIR; w.ln1 = w.ln2 = VS_LN_NONE; })},
    {"d 512, bf16 with bf16 attention: ring", rows(model(512, 8), 8193, BF16), defaults(), RING},
    {"d 1024 (head dim 128), bf16 with bf16 attention: ring", rows(model(1024, 8), 8193, BF16), defaults(), RING},
    {"d 512, bf16 Linear with exact attention: no ring", rows(model(512, 8), 8193, BF16_LIN), defaults(), WIDE_BF16_LIN},
    {"d 1024, bf16 Linear with exact attention: no ring", rows(model(1024, 8), 8193, BF16_LIN), defaults(), WIDE_BF16_LIN},
    {"d 512, bf16 at lp_min_rows: exact Linear, wide LayerNorm GEMMs", rows(model(512, 8), 8192, BF16), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.attention_arith = VS_ARITH_BF16; w.attention = VS_ATT_LOWPREC; w.mode_attention = 1; w.ln1 = w.ln2 = VS_LN_GEMM_ROWS; })},
    {"M-A, fp16x3", rows(MA, 320, F16X3), defaults(),
     Want{VS_ARITH_F16X3, VS_ARITH_F16X3, VSW_F16X3, VS_EMBED_GEMM, VS_ATT_LOWPREC, VS_LAYER_STAGES, VS_LN_FUSED, VS_LN_FUSED, false, false, false, false, 2, 2, 2, 2}},
    {"M-A, fp16x3 above skinny_rows: no image family", rows(MA, 16385, F16X3), defaults(),
     Want{VS_ARITH_F16X3, VS_ARITH_F16X3, 0, VS_EMBED_GEMM, VS_ATT_LOWPREC, VS_LAYER_STAGES, VS_LN_FUSED, VS_LN_FUSED, false, false, false, false, 2, 2, 2, 2}},
    {"head dim 256 (d 256, 1 head)", rows(model(256, 1), 320, 0), defaults(), but(EXACT_STAGES, [](Want &w) { w.attention = VS_ATT_DH256; })},
    // latency mode: the embedding splits K only where in_features is a multiple of 1024, the out-projection from d_model 256 on
    {"split-K, d 128, in_features 1024", rows(model(128, 4), 320, SPLITK), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.embed = VS_EMBED_SPLITK; w.attention = VS_ATT_SPLITKV; w.ln2 = VS_LN_SPLITK_ROWS; })},
    {"split-K, d 256, in_features 1024", rows(MA, 320, SPLITK), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.embed = VS_EMBED_SPLITK; w.attention = VS_ATT_SPLITKV; w.ln1 = w.ln2 = VS_LN_SPLITK_ROWS; })},
    {"split-K, d 512, in_features 1024", rows(model(512, 8), 320, SPLITK), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.embed = VS_EMBED_SPLITK; w.attention = VS_ATT_SPLITKV; w.ln1 = w.ln2 = VS_LN_SPLITK_ROWS; })},
    {"split-K, d 128, in_features 1000", rows(model(128, 4, 1000), 320, SPLITK), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.attention = VS_ATT_SPLITKV; w.ln2 = VS_LN_SPLITK_ROWS; })},
    {"split-K, d 256, in_features 1000", rows(model(256, 4, 1000), 320, SPLITK), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.attention = VS_ATT_SPLITKV; w.ln1 = w.ln2 = VS_LN_SPLITK_ROWS; })},
    {"split-K, d 512, in_features 1000", rows(model(512, 8, 1000), 320, SPLITK), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.attention = VS_ATT_SPLITKV; w.ln1 = w.ln2 = VS_LN_SPLITK_ROWS; })},
    {"split-K, fp16x3 Linear: the attention stays exact split-KV", rows(MA, 320, SPLITK | VS_FLAG_F16X3_LINEAR), defaults(),
     Want{VS_ARITH_F16X3, VS_ARITH_EXACT, VSW_F16X3, VS_EMBED_SPLITK, VS_ATT_SPLITKV, VS_LAYER_STAGES, VS_LN_SPLITK_ROWS, VS_LN_SPLITK_ROWS,
          false, false, false, false, 2, 2, 2, 0}},
    {"split-K refused: packed", packed(rows(MA, 320, SPLITK)), defaults(), but(EXACT_STAGES, [](Want &w) { w.attention = VS_ATT_PACKED; })},
    {"split-K refused: class token", with_cls(rows(MA, 320, SPLITK)), defaults(), but(EXACT_STAGES, [](Want &w) { w.embed = VS_EMBED_CLS; })},
    {"split-K refused: above skinny_rows", rows(MA, 16385, SPLITK), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.families = 0; w.layer = VS_LAYER_EXACT_PAIR; w.ln1 = w.ln2 = VS_LN_NONE; })},
    {"split-K refused: d 320", rows(model(320, 5), 320, SPLITK), defaults(), but(EXACT_STAGES, [](Want &w) { w.ln1 = w.ln2 = VS_LN_GEMM_ROWS; })},
    {"class token, B=2 x T=320", with_cls(call(MA, 2, 320, 0)), defaults(), but(EXACT_STAGES, [](Want &w) { w.embed = VS_EMBED_CLS; })},
    // the fragment-major copies follow the smallest GEMM of the forward: with a class token that is the embedding's B * T rows
    {"class token, B=2: 16384 frames, 16386 positions", with_cls(call(MA, 2, 8192, 0)), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.embed = VS_EMBED_CLS; w.layer = VS_LAYER_EXACT_PAIR; w.ln1 = w.ln2 = VS_LN_NONE; })},
    {"packed, exact attention", packed(rows(MA, 1000, 0)), defaults(), but(EXACT_STAGES, [](Want &w) { w.attention = VS_ATT_PACKED; })},
    {"packed, bf16 attention alone", packed(rows(MA, 1000, BF16_ATT)), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.attention_arith = VS_ARITH_BF16; w.attention = VS_ATT_PACKED; w.mode_attention = 1; })},
    {"packed, bf16", packed(rows(MA, 1000, BF16)), defaults(), but(BF16_FUSED, [](Want &w) { w.attention = VS_ATT_PACKED; })},
    {"packed, fp16x3 attention", packed(rows(MA, 1000, VS_FLAG_F16X3_ATTENTION)), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.attention_arith = VS_ARITH_F16X3; w.attention = VS_ATT_PACKED; w.mode_attention = 2; })},
    {"packed, d 512, bf16: no ring", packed(rows(model(512, 8), 8193, BF16)), defaults(),
     but(WIDE_BF16_LIN, [](Want &w) { w.attention_arith = VS_ARITH_BF16; w.attention = VS_ATT_PACKED; w.mode_attention = 1; })},
    // head dim 128 at d_model <= 256: q/k/v are bf16 planes there too, so the packed attention is asked for its bf16-stored form
    {"packed, d 256 x 2 heads (head dim 128), bf16", packed(rows(model(256, 2), 1000, BF16)), defaults(),
     but(BF16_FUSED, [](Want &w) { w.attention = VS_ATT_PACKED; })},
    {"packed, d 128 x 1 head (head dim 128), bf16", packed(rows(model(128, 1), 8193, BF16)), defaults(),
     Want{VS_ARITH_BF16, VS_ARITH_BF16, VSW_BF16, VS_EMBED_GEMM, VS_ATT_PACKED, VS_LAYER_STAGES, VS_LN_FUSED, VS_LN_FUSED, true, true, false, true, 1, S16, S16, S16}},
    // latency mode, wider embeddings: an eighth of in_features has to be a slice vsk_linear_parts takes (3072 / 8 = 384 is not)
    {"split-K, d 256, in_features 2048", rows(model(256, 4, 2048), 320, SPLITK), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.embed = VS_EMBED_SPLITK; w.attention = VS_ATT_SPLITKV; w.ln1 = w.ln2 = VS_LN_SPLITK_ROWS; })},
    {"split-K, d 256, in_features 3072: default embedding", rows(model(256, 4, 3072), 320, SPLITK), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.attention = VS_ATT_SPLITKV; w.ln1 = w.ln2 = VS_LN_SPLITK_ROWS; })},
    {"split-K, d 512, in_features 5120: default embedding", rows(model(512, 8, 5120), 320, SPLITK), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.attention = VS_ATT_SPLITKV; w.ln1 = w.ln2 = VS_LN_SPLITK_ROWS; })},
    // an embedded model's LayerNorm is narrower than its rows: no fused kernel normalises it, and nothing is stored as bf16
    {"embedded model, bf16", embedded(rows(MA, 8193, BF16)), defaults(),
     Want{VS_ARITH_BF16, VS_ARITH_BF16, VSW_BF16, VS_EMBED_GEMM, VS_ATT_LOWPREC, VS_LAYER_STAGES, VS_LN_GEMM_ROWS, VS_LN_GEMM_ROWS, false, false, false, false, 1, 1, 1, 1}},
    {"embedded model, bf16 at lp_min_rows_fused + 1: the fused threshold does not apply", embedded(rows(MA, 257, BF16)), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.attention_arith = VS_ARITH_BF16; w.attention = VS_ATT_LOWPREC; w.mode_attention = 1; w.ln1 = w.ln2 = VS_LN_GEMM_ROWS; })},
    {"embedded model, exact above skinny_rows: no fused pair", embedded(rows(MA, 16385, 0)), defaults(),
     but(EXACT_STAGES, [](Want &w) { w.families = 0; w.ln1 = w.ln2 = VS_LN_GEMM_ROWS; })},
    // the three thresholds pinned to 0, as the GPU tests do
    {"VS_SKINNY_ROWS=0: exact fused pair at 320 rows", rows(MA, 320, 0), with(&VskOptions::skinny_rows, 0),
     but(EXACT_STAGES, [](Want &w) { w.families = 0; w.layer = VS_LAYER_EXACT_PAIR; w.ln1 = w.ln2 = VS_LN_NONE; })},
    {"VS_LP_MIN_ROWS=0: bf16 Linear at 65 rows", rows(MA, 65, BF16_LIN), with(&VskOptions::lp_min_rows, 0), BF16_LIN_MA},
    {"VS_LP_MIN_ROWS_FUSED=0: fused bf16 at 65 rows", rows(MA, 65, BF16), with(&VskOptions::lp_min_rows_fused, 0), BF16_FUSED},
    {"no bf16 embedding image (in_features 1000): generic embedding, first QKV by vsk_qkv", rows(model(256, 4, 1000), 1000, BF16), defaults(),
     but(BF16_FUSED, [](Want &w) { w.embed = VS_EMBED_GEMM; })},
};

// ---- part 2: each switch against its base case ("acts on") ----
struct Flip { const char *name; int VskOptions::*field; VsForwardIn in; Want base, flipped; unsigned fields; };
const VsForwardIn LP = rows(MA, 8193, BF16);       // above both bf16 thresholds, so a switch cannot move the Linear arithmetic
const Flip kFlips[] = {
    {"VS_LP_STORE32", &VskOptions::lp_store32, LP, BF16_FUSED,
     Want{VS_ARITH_BF16, VS_ARITH_BF16, VSW_BF16, VS_EMBED_GEMM, VS_ATT_LOWPREC, VS_LAYER_STAGES, VS_LN_FUSED, VS_LN_FUSED, false, false, false, false, 1, 1, 1, 1},
     bit(F_EMBED) | bit(F_LAYER) | bit(F_LN1) | bit(F_LN2) | bit(F_QKV16) | bit(F_FFN16) | bit(F_NEXT_QKV) | bit(F_KV_STRIDE) | bit(F_MODE_QKV) |
         bit(F_MODE_FFN) | bit(F_MODE_ATT)},
    {"VS_LP_MLP_UNFUSED", &VskOptions::lp_mlp_unfused, LP, BF16_FUSED,
     but(BF16_FUSED, [](Want &w) { w.embed = VS_EMBED_GEMM; w.layer = VS_LAYER_STAGES; w.ln1 = w.ln2 = VS_LN_FUSED; w.next_qkv = false; }),
     bit(F_EMBED) | bit(F_LAYER) | bit(F_LN1) | bit(F_LN2) | bit(F_NEXT_QKV)},
    {"VS_LP_TAIL_UNFUSED", &VskOptions::lp_tail_unfused, LP, BF16_FUSED,
     but(BF16_FUSED, [](Want &w) { w.layer = VS_LAYER_BF16_MLP; w.ln1 = VS_LN_FUSED; }), bit(F_LAYER) | bit(F_LN1)},
    {"VS_LP_QKV_UNFUSED", &VskOptions::lp_qkv_unfused, LP, BF16_FUSED,
     but(BF16_FUSED, [](Want &w) { w.embed = VS_EMBED_GEMM; w.next_qkv = false; }), bit(F_EMBED) | bit(F_NEXT_QKV)},
    {"VS_LP_EMBED_UNFUSED", &VskOptions::lp_embed_unfused, LP, BF16_FUSED, but(BF16_FUSED, [](Want &w) { w.embed = VS_EMBED_GEMM; }), bit(F_EMBED)},
    {"VS_EXACT_UNFUSED", &VskOptions::exact_unfused, rows(MA, 16385, 0),
     but(EXACT_STAGES, [](Want &w) { w.families = 0; w.layer = VS_LAYER_EXACT_PAIR; w.ln1 = w.ln2 = VS_LN_NONE; }),
     but(EXACT_STAGES, [](Want &w) { w.families = 0; }), bit(F_LAYER) | bit(F_LN1) | bit(F_LN2)},
};

// ---- part 3: the refusal the documented rules give for `in` (empty: none), in their order of precedence ----
std::string expected_refusal(const VsForwardIn &in) {
    char msg[192] = "";
    const int dh = in.d_model / in.num_heads;
    const unsigned f = in.flags;
    if (!in.packed && in.has_pe && in.T > in.max_len) snprintf(msg, sizeof msg, "T=%d exceeds the positional table (max_len=%d)", in.T, in.max_len);
    else if (in.cls && in.packed) snprintf(msg, sizeof msg, "packed batches have no class-token form");
    else if ((long long)in.B * (in.T + (in.cls ? 1 : 0)) > (1ll << 30)) snprintf(msg, sizeof msg, "B*T too large");
    else if ((f & VS_FLAG_BF16_LINEAR) && (f & VS_FLAG_F16X3_LINEAR)) snprintf(msg, sizeof msg, "VS_FLAG_BF16_LINEAR and VS_FLAG_F16X3_LINEAR are exclusive");
    else if (((f & (VS_FLAG_BF16_ATTENTION | VS_FLAG_F16X3_ATTENTION)) && dh == 256) || ((f & VS_FLAG_F16X3_ATTENTION) && !(f & VS_FLAG_BF16_ATTENTION) && dh == 128))
        snprintf(msg, sizeof msg, "VS_FLAG_BF16_ATTENTION needs head_dim 32, 64 or 128, VS_FLAG_F16X3_ATTENTION 32 or 64 (got %d)", dh);
    else if ((f & VS_FLAG_BF16_ATTENTION) && (f & VS_FLAG_F16X3_ATTENTION)) snprintf(msg, sizeof msg, "VS_FLAG_BF16_ATTENTION and VS_FLAG_F16X3_ATTENTION are exclusive");
    else if (in.packed && dh == 256) snprintf(msg, sizeof msg, "packed batches need head_dim 32, 64 or 128 (got %d)", dh);     // no packed attention kernel
    return msg;
}

// every kernel an accepted plan names exists: the support predicate of each launcher it sends forward_core to holds (the
// attention launchers of the padded forms have no predicate: their head-dim rules are restated here)
int kernels_exist(const VsForwardIn &in, const VskOptions &opt, const VsForwardPlan &p) {
    const int d = in.d_model, dh = d / in.num_heads;
    switch (p.attention) {
    case VS_ATT_PACKED: {     // the tiling is a fact of the lengths: both answers vs_packed_waves has, from lengths that give them
        const long long tilings[][2] = {{1024, 1024}, {105, 100}, {106, 100}, {256, 128}};
        for (auto &t : tilings) CHECK(vsk_attention_packed_supported(dh, vs_packed_waves(dh, p.attention_arith, t[0], t[1]), p.mode_attention));
    } break;
    case VS_ATT_DH256: CHECK(dh == 256 && p.mode_attention == 0); break;
    case VS_ATT_SPLITKV: CHECK((dh == 32 || dh == 64 || dh == 128) && p.attention_arith != VS_ARITH_BF16); break;      // (exact whatever the word says)
    case VS_ATT_LOWPREC: CHECK(dh == 32 || dh == 64 || (dh == 128 && p.mode_attention != 2)); CHECK(p.mode_attention == 1 || p.mode_attention == 2 || p.mode_attention == S16); break;
    case VS_ATT_EXACT: CHECK((dh == 32 || dh == 64 || dh == 128) && p.mode_attention == 0); break;
    }
    if (p.embed == VS_EMBED_SPLITK) CHECK(vsk_linear_parts_supported(d, in.in_features, 8));
    if (p.ln1 == VS_LN_SPLITK_ROWS) CHECK(vsk_linear_parts_supported(d, d, 2));
    if (p.ln2 == VS_LN_SPLITK_ROWS) CHECK(vsk_linear_parts_supported(d, 4 * d, 4));
    if (p.embed == VS_EMBED_BF16_QKV) CHECK(vsk_mlp_bf16_supported(d) && in.has_b_embed);
    if (p.layer == VS_LAYER_BF16_TAIL || p.layer == VS_LAYER_BF16_MLP) CHECK(vsk_mlp_bf16_supported(d));
    if (p.layer == VS_LAYER_RING)
        CHECK(vsk_gemm16_supported(p.M, 3 * d, d) && vsk_gemm16_supported(p.M, d, d) && vsk_gemm16_supported(p.M, 4 * d, d) && vsk_gemm16_supported(p.M, d, 4 * d));
    if (p.layer == VS_LAYER_EXACT_PAIR) CHECK(vsk_layer_fused_supported(p.M, d, opt.skinny_rows));
    return 0;
}

// latency mode over embedding widths: the embedding splits K exactly where vsk_linear_parts takes an eighth of in_features
int latency_grid(const int (*dims)[2], int ndims, long long *points) {
    const int widths[] = {1000, 1024, 2048, 3072, 4096, 5120};
    const int frames[] = {65, 320};
    const unsigned modes[] = {SPLITK, SPLITK | VS_FLAG_F16X3_LINEAR};
    for (int i = 0; i < ndims; ++i) for (int w : widths) for (int T : frames) for (unsigned flags : modes) for (int kind = 0; kind < 3; ++kind) {
        VsForwardIn in = rows(model(dims[i][0], dims[i][1], w), T, flags);
        if (kind == 1) in = with_cls(in);
        if (kind == 2) in = packed(in);
        VsForwardPlan p;
        std::string err;
        const int rc = vs_forward_plan(in, defaults(), &p, &err);
        ++*points;
        if (!expected_refusal(in).empty()) { CHECK(rc == VS_ERR_INVALID && err == expected_refusal(in)); continue; }
        CHECK(rc == VS_OK);
        if (kernels_exist(in, defaults(), p)) { std::printf("  (latency grid: d %d, %d heads, in_features %d, T %d, flags %u, kind %d)\n", dims[i][0], dims[i][1], w, T, flags, kind); return 1; }
        const int d = dims[i][0];
        const bool latency = kind == 0 && (d == 128 || d == 256 || d == 512);
        CHECK((p.ln2 == VS_LN_SPLITK_ROWS) == latency);
        CHECK((p.embed == VS_EMBED_SPLITK) == (latency && (w == 1024 || w == 2048 || w == 4096)));
    }
    return 0;
}

int grid(long long *points) {
    const int dims[][2] = {{128, 4}, {128, 2}, {128, 1}, {256, 8}, {256, 4}, {256, 2}, {256, 1}, {320, 10}, {320, 5},
                           {512, 16}, {512, 8}, {512, 4}, {512, 2}, {1024, 32}, {1024, 16}, {1024, 8}, {1024, 4}};      // head dim 32 .. 256
    const int bt[][2] = {{1, 255}, {1, 256}, {1, 257}, {4, 64}, {4, 65}, {8, 1024}, {1, 8193}, {2, 8192}, {16385, 1}, {1, 20001}, {32769, 32768}};
    int VskOptions::*const switches[] = {nullptr, &VskOptions::lp_store32, &VskOptions::lp_mlp_unfused, &VskOptions::lp_tail_unfused,
                                         &VskOptions::lp_qkv_unfused, &VskOptions::lp_embed_unfused, &VskOptions::exact_unfused,
                                         &VskOptions::skinny_rows, &VskOptions::lp_min_rows, &VskOptions::lp_min_rows_fused};
    for (auto &dm : dims) for (auto &s : bt) for (unsigned flags = 0; flags < 64; ++flags) for (auto sw : switches) for (int kind = 0; kind < 3; ++kind)
        for (int emb = 0; emb < 2; ++emb) {
            VsForwardIn in = call(model(dm[0], dm[1]), s[0], s[1], flags);
            if (kind == 1) in = with_cls(in);
            if (kind == 2) in = packed(in);
            if (emb) in = embedded(in);
            VskOptions opt = defaults();
            if (sw) opt.*sw = (sw == &VskOptions::skinny_rows || sw == &VskOptions::lp_min_rows || sw == &VskOptions::lp_min_rows_fused) ? 0 : 1;
            VsForwardPlan p, untouched;
            std::memset((void *)&p, 0x5a, sizeof p);
            std::memcpy((void *)&untouched, (const void *)&p, sizeof p);
            std::string err;
            const int rc = vs_forward_plan(in, opt, &p, &err);
            ++*points;
            const std::string refusal = expected_refusal(in);
            if (!refusal.empty()) {     // the documented error, and no plan
                CHECK(rc == VS_ERR_INVALID && err == refusal && std::memcmp((const void *)&p, (const void *)&untouched, sizeof p) == 0);
                continue;
            }
            CHECK(rc == VS_OK && err.empty());
            const size_t plane = (size_t)p.M * in.d_model;
            const bool ring = p.layer == VS_LAYER_RING, tail_family = p.layer == VS_LAYER_BF16_TAIL || p.layer == VS_LAYER_BF16_MLP;
            CHECK(p.T == in.T + (in.cls ? 1 : 0) && p.M == in.B * p.T);
            // exactly one layer form, and the two LayerNorm stages are named exactly where that form has them as stages
            CHECK(p.layer == VS_LAYER_RING || p.layer == VS_LAYER_BF16_TAIL || p.layer == VS_LAYER_BF16_MLP || p.layer == VS_LAYER_EXACT_PAIR || p.layer == VS_LAYER_STAGES);
            CHECK((p.layer == VS_LAYER_STAGES) == (p.ln1 != VS_LN_NONE && p.ln2 != VS_LN_NONE));
            CHECK((p.layer == VS_LAYER_BF16_MLP) == (p.ln1 != VS_LN_NONE && p.ln2 == VS_LN_NONE));
            CHECK(p.layer != VS_LAYER_BF16_MLP || p.ln1 == VS_LN_FUSED);
            CHECK(p.ln1 != VS_LN_NONE || p.ln2 == VS_LN_NONE);
            CHECK(!p.next_qkv || (p.qkv16 && tail_family));
            CHECK(p.embed != VS_EMBED_BF16_QKV || p.next_qkv);
            CHECK(!ring || (!p.qkv16 && (p.families & VSW_ROWS16)));
            CHECK((p.linear == VS_ARITH_BF16) == ((p.families & VSW_BF16) != 0));
            CHECK(!(ring || tail_family || p.embed == VS_EMBED_BF16_QKV || p.qkv16 || p.ffn16) || p.linear == VS_ARITH_BF16);
            CHECK(p.kv_stride == ((p.qkv16 || ring) ? plane / 2 : plane));
            CHECK(!p.qkv16 || (p.ffn16 && p.attention_arith == VS_ARITH_BF16));
            // the mode words say what the storage facts say
            CHECK(p.mode_linear == p.linear && p.mode_qkv == (p.qkv16 ? S16 : p.linear) && p.mode_ffn == (p.ffn16 ? S16 : p.linear));
            CHECK(p.mode_attention == ((p.qkv16 || ring) ? S16 : p.attention_arith));
            // the exact kernels (and the attention-map hook) read fp32 planes
            CHECK(!(p.attention == VS_ATT_EXACT || p.attention == VS_ATT_DH256 || p.attention == VS_ATT_SPLITKV) || p.kv_stride == plane);
            CHECK((p.attention == VS_ATT_PACKED) == in.packed && (p.embed == VS_EMBED_CLS) == in.cls);
            CHECK(p.layer != VS_LAYER_EXACT_PAIR || (p.linear == VS_ARITH_EXACT && p.attention_arith == VS_ARITH_EXACT && p.M > opt.skinny_rows));
            // latency mode: only with the flag, never packed, with a class token, in bf16 or above the skinny threshold
            const bool latency = p.embed == VS_EMBED_SPLITK || p.attention == VS_ATT_SPLITKV || p.ln1 == VS_LN_SPLITK_ROWS || p.ln2 == VS_LN_SPLITK_ROWS;
            CHECK(!latency || ((flags & VS_FLAG_SPLITK) && !in.packed && !in.cls && p.linear != VS_ARITH_BF16 && p.M <= opt.skinny_rows && p.ln2 == VS_LN_SPLITK_ROWS));
            if (emb) CHECK(!p.qkv16 && !p.ffn16 && !tail_family && p.layer != VS_LAYER_EXACT_PAIR && p.ln1 != VS_LN_FUSED && p.ln2 != VS_LN_FUSED);
            if (kernels_exist(in, opt, p)) {
                std::printf("  (grid: d %d, %d heads, B %d, T %d, flags %u, kind %d, embedded %d)\n", dm[0], dm[1], s[0], s[1], flags, kind, emb);
                return 1;
            }
        }
    return latency_grid(dims, (int)(sizeof dims / sizeof dims[0]), points);
}

}  // namespace

int main() {
    for (const Case &c : kCases) CHECK(plan_is(c));
    const int enumerators[] = {3, 3, 4, 5, 5, 4};       // VsArith (Linear), VsArith (attention), VsEmbedForm, VsAttentionKernel, VsLayerForm, VsLnForm
    for (int e = 0; e < 6; ++e)
        for (int v = 0; v < enumerators[e]; ++v)
            if (!g_seen.count({e, v})) { std::printf("FAILED: no named case reaches enumerator %d of plan enum %d\n", v, e); return 1; }

    for (const Flip &f : kFlips) {
        CHECK(plan_is(Case{f.name, f.in, defaults(), f.base}));
        CHECK(plan_is(Case{f.name, f.in, with(f.field, 1), f.flipped}));
        VsForwardPlan a, b;
        std::string err;
        CHECK(vs_forward_plan(f.in, defaults(), &a, &err) == VS_OK && vs_forward_plan(f.in, with(f.field, 1), &b, &err) == VS_OK);
        if (differing(a, b) != f.fields) { std::printf("FAILED: %s flips fields 0x%x, documented 0x%x\n", f.name, differing(a, b), f.fields); return 1; }
    }

    {   // refusals: code, text, order of precedence
        VsForwardPlan p;
        std::string err;
        VsForwardIn in = rows(model(256, 1), 20001, VS_FLAG_BF16 | VS_FLAG_F16X3);      // every rule at once: the first one speaks
        CHECK(vs_forward_plan(in, defaults(), &p, &err) == VS_ERR_INVALID && err == "T=20001 exceeds the positional table (max_len=20000)");
        in.has_pe = false;                                                              // no positional table: any T
        CHECK(vs_forward_plan(in, defaults(), &p, &err) == VS_ERR_INVALID && err == "VS_FLAG_BF16_LINEAR and VS_FLAG_F16X3_LINEAR are exclusive");
        in.flags = VS_FLAG_BF16_ATTENTION | VS_FLAG_F16X3_ATTENTION;
        CHECK(vs_forward_plan(in, defaults(), &p, &err) == VS_ERR_INVALID &&
              err == "VS_FLAG_BF16_ATTENTION needs head_dim 32, 64 or 128, VS_FLAG_F16X3_ATTENTION 32 or 64 (got 256)");
        CHECK(vs_forward_plan(rows(MA, 320, VS_FLAG_BF16_ATTENTION | VS_FLAG_F16X3_ATTENTION), defaults(), &p, &err) == VS_ERR_INVALID &&
              err == "VS_FLAG_BF16_ATTENTION and VS_FLAG_F16X3_ATTENTION are exclusive");
        CHECK(vs_forward_plan(rows(model(1024, 8), 320, VS_FLAG_F16X3_ATTENTION), defaults(), &p, &err) == VS_ERR_INVALID);      // head dim 128: bf16 only
        CHECK(vs_forward_plan(rows(model(1024, 8), 320, VS_FLAG_BF16_ATTENTION), defaults(), &p, &err) == VS_OK);
        CHECK(vs_forward_plan(with_cls(packed(rows(MA, 320, 0))), defaults(), &p, &err) == VS_ERR_INVALID && err == "packed batches have no class-token form");
        CHECK(vs_forward_plan(call(MA, 1 << 16, 1 << 14, 0), defaults(), &p, &err) == VS_OK);                                     // B * T == 2^30
        CHECK(vs_forward_plan(with_cls(call(MA, 1 << 16, 1 << 14, 0)), defaults(), &p, &err) == VS_ERR_INVALID && err == "B*T too large");
        CHECK(vs_forward_plan(packed(rows(MA, 20001, 0)), defaults(), &p, &err) == VS_OK);      // a packed batch's T is all its frames: the entry checks each video
    }

    // packed batches: the query tile in waves.  256-row tiles while they waste at most 5 % more rows than 128-row tiles
    CHECK(vs_packed_waves(64, 0, 1024, 1024) == 8 && vs_packed_waves(64, 0, 105, 100) == 8 && vs_packed_waves(64, 0, 106, 100) == 4);
    CHECK(vs_packed_waves(64, 1, 1024, 1024) == 8 && vs_packed_waves(64, 2, 1024, 1024) == 8);
    CHECK(vs_packed_waves(32, 0, 1024, 1024) == 8 && vs_packed_waves(32, 1, 1024, 1024) == 4 && vs_packed_waves(32, 2, 1024, 1024) == 4);
    CHECK(vs_packed_waves(128, 0, 1024, 1024) == 4 && vs_packed_waves(128, 1, 1024, 1024) == 8 && vs_packed_waves(128, 1, 256, 128) == 8);

    // ... and the kernels vsk_attention_packed has for them, per mode word: bf16 at head dim 128 on 8-wave blocks in both storage forms
    CHECK(vsk_attention_packed_supported(128, 8, S16) && vsk_attention_packed_supported(128, 8, 1) && vsk_attention_packed_supported(128, 4, 0));
    CHECK(!vsk_attention_packed_supported(128, 4, S16) && !vsk_attention_packed_supported(128, 4, 1) && !vsk_attention_packed_supported(128, 8, 0));
    CHECK(!vsk_attention_packed_supported(128, 8, 2) && !vsk_attention_packed_supported(128, 4, 2) && !vsk_attention_packed_supported(256, 4, 0));
    CHECK(vsk_attention_packed_supported(32, 8, 0) && !vsk_attention_packed_supported(32, 8, 1) && !vsk_attention_packed_supported(32, 8, 2) && !vsk_attention_packed_supported(32, 8, S16));
    CHECK(!vsk_attention_packed_supported(64, 2, 0) && !vsk_attention_packed_supported(64, 8, 3) && !vsk_attention_packed_supported(48, 4, 0));
    // split-K slices: multiples of 128, whole 256-k phases above 256
    CHECK(vsk_linear_parts_supported(256, 1024, 8) && vsk_linear_parts_supported(256, 2048, 8) && vsk_linear_parts_supported(256, 4096, 8));
    CHECK(!vsk_linear_parts_supported(256, 3072, 8) && !vsk_linear_parts_supported(256, 5120, 8) && !vsk_linear_parts_supported(256, 1000, 8));
    CHECK(!vsk_linear_parts_supported(250, 1024, 8) && !vsk_linear_parts_supported(256, 1024, 0) && !vsk_linear_parts_supported(256, 1024, 3));

    long long points = 0;
    if (grid(&points)) return 1;
    std::printf("OK\n");
    return 0;
}
